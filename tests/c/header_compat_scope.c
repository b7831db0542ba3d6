/* header_compat_scope.c -- the scoped-find entry points of include/blurrily_storage.h (blurrily_scope_* and
 * blurrily_storage_find_in / _find_batch_in[_device]) in ONE translation unit with the reference's ext/blurrily/storage.h,
 * compiled with -std=c99 -Wall -Wextra -Werror by tests/test_scope_abi.py.  "storage.h" is the stand-in made from
 * tests/golden/ref_abi.json (the header is never copied).  The reference has no scoped find, so nothing of its own may
 * clash with these prototypes, and the types they use must be the ones both headers agree on. */
#include "storage.h"
#include "blurrily_storage.h"

int scope_compat_calls(trigram_map m, const uint32_t* refs, const char* packed, const uint64_t* offsets,
                       trigram_match rows, uint32_t* counts);
int scope_compat_calls(trigram_map m, const uint32_t* refs, const char* packed, const uint64_t* offsets,
                       trigram_match rows, uint32_t* counts)
{
  int (*f_new)(trigram_map, const uint32_t*, size_t, blurrily_scope*) = blurrily_scope_new;
  int (*f_close)(blurrily_scope*) = blurrily_scope_close;
  int (*f_members)(blurrily_scope, uint32_t*) = blurrily_scope_members;
  int (*f_find)(trigram_map, blurrily_scope, const char*, uint16_t, trigram_match) = blurrily_storage_find_in;
  int (*f_batch)(trigram_map, blurrily_scope, const char*, const uint64_t*, size_t, uint16_t, trigram_match,
                 uint32_t*) = blurrily_storage_find_batch_in;
  int (*f_dev)(trigram_map, blurrily_scope, const char*, size_t, const uint64_t*, size_t, uint16_t, trigram_match,
               uint32_t*, void*) = blurrily_storage_find_batch_in_device;
  blurrily_scope scope = NULL;
  uint32_t held = 0;
  int r = f_new(m, refs, 2, &scope);
  r += f_members(scope, &held);
  r += f_find(m, scope, "london", 10, rows);
  r += f_batch(m, scope, packed, offsets, 1, 10, rows, counts);
  r += f_dev(m, scope, packed, 6, offsets, 1, 10, rows, counts, NULL);
  r += f_close(&scope);
  return r + (int)held;
}

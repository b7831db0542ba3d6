/* header_compat_scope_each.c -- the scope-per-needle entry points of include/blurrily_storage.h
 * (blurrily_storage_find_batch_each_in[_device], _find_references_each_in, BLURRILY_NO_SCOPE) in ONE translation unit
 * with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by
 * tests/test_scope_each_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is never
 * copied).  The reference has no scoped find, so nothing of its own may clash with these prototypes. */
#include "storage.h"
#include "blurrily_storage.h"

int scope_each_compat_calls(trigram_map m, const blurrily_scope* scopes, const uint32_t* refs, const char* packed,
                            const uint64_t* offsets, trigram_match rows, uint32_t* counts);
int scope_each_compat_calls(trigram_map m, const blurrily_scope* scopes, const uint32_t* refs, const char* packed,
                            const uint64_t* offsets, trigram_match rows, uint32_t* counts)
{
  int (*f_batch)(trigram_map, const blurrily_scope*, size_t, const uint32_t*, const char*, const uint64_t*, size_t,
                 uint16_t, trigram_match, uint32_t*) = blurrily_storage_find_batch_each_in;
  int (*f_dev)(trigram_map, const blurrily_scope*, size_t, const uint32_t*, const char*, size_t, const uint64_t*,
               size_t, uint16_t, trigram_match, uint32_t*, void*) = blurrily_storage_find_batch_each_in_device;
  int (*f_refs)(trigram_map, const blurrily_scope*, size_t, const uint32_t*, const uint32_t*, size_t, uint16_t,
                trigram_match, uint32_t*, uint32_t*) = blurrily_storage_find_references_each_in;
  const uint32_t which[2] = {0u, BLURRILY_NO_SCOPE};
  uint32_t nb[2] = {0u, 0u};
  int r = f_batch(m, scopes, 1, which, packed, offsets, 2, 10, rows, counts);
  r += f_dev(m, scopes, 1, which, packed, 12, offsets, 2, 10, rows, counts, NULL);
  r += f_refs(m, scopes, 1, which, refs, 2, 10, rows, counts, nb);
  return r + (int)nb[0] + (BLURRILY_NO_SCOPE == 0xFFFFFFFFu ? 0 : 1);
}

/* header_compat_scope_above.c -- the scoped threshold find's entry points of include/blurrily_storage.h
 * (blurrily_storage_find_batch_above_in, _find_above_in, _find_batch_above_each_in, _find_references_above_each_in) in
 * ONE translation unit with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by
 * tests/test_scope_above_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is never
 * copied).  The reference has neither scopes nor a threshold find, so nothing of its own may clash with these
 * prototypes. */
#include "storage.h"
#include "blurrily_storage.h"

int scope_above_compat_calls(trigram_map m, blurrily_scope sc, const uint32_t* refs, const char* packed,
                             const uint64_t* offsets, trigram_match rows);
int scope_above_compat_calls(trigram_map m, blurrily_scope sc, const uint32_t* refs, const char* packed,
                             const uint64_t* offsets, trigram_match rows)
{
  int (*f_batch)(trigram_map, blurrily_scope, const char*, const uint64_t*, size_t, uint32_t, uint32_t, trigram_match,
                 uint64_t, uint64_t*) = blurrily_storage_find_batch_above_in;
  int (*f_one)(trigram_map, blurrily_scope, const char*, uint32_t, uint32_t, trigram_match, uint64_t, uint64_t*) =
      blurrily_storage_find_above_in;
  int (*f_each)(trigram_map, const blurrily_scope*, size_t, const uint32_t*, const char*, const uint64_t*, size_t,
                uint32_t, uint32_t, trigram_match, uint64_t, uint64_t*) = blurrily_storage_find_batch_above_each_in;
  int (*f_refs)(trigram_map, const blurrily_scope*, size_t, const uint32_t*, const uint32_t*, size_t, uint32_t,
                uint32_t, trigram_match, uint64_t, uint64_t*, uint32_t*) =
      blurrily_storage_find_references_above_each_in;
  const blurrily_scope scopes[1] = {sc};
  const uint32_t which[2] = {0u, BLURRILY_NO_SCOPE};
  uint64_t row_off[3] = {0u, 0u, 0u};
  uint64_t total = 0u;
  uint32_t nb[2] = {0u, 0u};
  int r = f_batch(m, sc, packed, offsets, 2, 0u, 700u, rows, 16u, row_off);
  r += f_one(m, sc, "needle", 3u, 0u, rows, 16u, &total);
  r += f_each(m, scopes, 1, which, packed, offsets, 2, 0u, 500u, rows, 16u, row_off);
  r += f_refs(m, scopes, 1, which, refs, 2, 2u, 800u, NULL, 0u, row_off, nb);
  return r + (int)nb[0] + (int)row_off[2] + (int)total;
}

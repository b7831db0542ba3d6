/* header_compat_above.c -- the threshold find's entry points of include/blurrily_storage.h
 * (blurrily_storage_find_batch_above, _find_above, _find_references_above) in ONE translation unit with the
 * reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by tests/test_above_abi.py.
 * "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is never copied).  The reference has no
 * threshold find, so nothing of its own may clash with these prototypes. */
#include "storage.h"
#include "blurrily_storage.h"

int above_compat_calls(trigram_map m, const uint32_t* refs, const char* packed, const uint64_t* offsets,
                       trigram_match rows);
int above_compat_calls(trigram_map m, const uint32_t* refs, const char* packed, const uint64_t* offsets,
                       trigram_match rows)
{
  int (*f_batch)(trigram_map, const char*, const uint64_t*, size_t, uint32_t, uint32_t, trigram_match, uint64_t,
                 uint64_t*) = blurrily_storage_find_batch_above;
  int (*f_one)(trigram_map, const char*, uint32_t, uint32_t, trigram_match, uint64_t, uint64_t*) =
      blurrily_storage_find_above;
  int (*f_refs)(trigram_map, const uint32_t*, size_t, uint32_t, uint32_t, trigram_match, uint64_t, uint64_t*,
                uint32_t*) = blurrily_storage_find_references_above;
  uint64_t off[3] = {0u, 0u, 0u};
  uint64_t total = 0u;
  uint32_t nb[2] = {0u, 0u};
  int r = f_batch(m, packed, offsets, 2, 2u, 700u, rows, 16u, off);
  r += f_batch(m, packed, offsets, 2, 0u, 500u, NULL, 0u, off);
  r += f_one(m, "needle", 0u, 700u, rows, 16u, &total);
  r += f_refs(m, refs, 2, 0u, 800u, rows, 16u, off, nb);
  return r + (int)nb[0] + (int)total + (int)off[2];
}

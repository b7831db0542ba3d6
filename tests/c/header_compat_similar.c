/* header_compat_similar.c -- the similarity find's entry points of include/blurrily_storage.h
 * (blurrily_storage_find_batch_similar, _find_similar, _find_references_similar) in ONE translation unit with the
 * reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by tests/test_similar_abi.py.
 * "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is never copied).  The reference has no
 * similarity find, so nothing of its own may clash with these prototypes. */
#include "storage.h"
#include "blurrily_storage.h"

int similar_compat_calls(trigram_map m, const uint32_t* refs, const char* packed, const uint64_t* offsets,
                         trigram_match rows);
int similar_compat_calls(trigram_map m, const uint32_t* refs, const char* packed, const uint64_t* offsets,
                         trigram_match rows)
{
  int (*f_batch)(trigram_map, const char*, const uint64_t*, size_t, uint16_t, uint32_t, trigram_match, uint32_t*,
                 uint32_t*) = blurrily_storage_find_batch_similar;
  int (*f_one)(trigram_map, const char*, uint16_t, uint32_t, trigram_match, uint32_t*) =
      blurrily_storage_find_similar;
  int (*f_refs)(trigram_map, const uint32_t*, size_t, uint16_t, uint32_t, trigram_match, uint32_t*, uint32_t*,
                uint32_t*) = blurrily_storage_find_references_similar;
  uint32_t counts[2] = {0u, 0u};
  uint32_t ntri[16] = {0u};
  uint32_t nb[2] = {0u, 0u};
  int r = f_batch(m, packed, offsets, 2, 8u, 700u, rows, counts, ntri);
  r += f_batch(m, packed, offsets, 2, 8u, 500u, rows, counts, NULL);
  r += f_one(m, "needle", 10u, 300u, rows, ntri);
  r += f_refs(m, refs, 2, 8u, 800u, rows, counts, ntri, nb);
  return r + (int)nb[0] + (int)counts[1] + (int)ntri[0];
}

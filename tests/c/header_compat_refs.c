/* header_compat_refs.c -- the by-reference entry points of include/blurrily_storage.h (blurrily_storage_get and the
 * find by reference) in ONE translation unit with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall
 * -Wextra -Werror by tests/test_refs_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the
 * header is never copied).  The reference's storage.h:72-87 only comments blurrily_storage_get out, so nothing of its
 * own may clash with these prototypes, and the types they use must be the ones both headers agree on. */
#include "storage.h"
#include "blurrily_storage.h"

int refs_compat_calls(trigram_map m, const uint32_t* refs, trigram_match rows, uint32_t* counts);
int refs_compat_calls(trigram_map m, const uint32_t* refs, trigram_match rows, uint32_t* counts)
{
  int (*f_get)(trigram_map, uint32_t, uint32_t*, int, uint16_t*) = blurrily_storage_get;
  int (*f_get_batch)(trigram_map, const uint32_t*, size_t, uint32_t*, uint64_t*, uint16_t*, size_t) =
      blurrily_storage_get_batch;
  int (*f_find)(trigram_map, const uint32_t*, size_t, uint16_t, trigram_match, uint32_t*, uint32_t*) =
      blurrily_storage_find_references;
  int (*f_find_dev)(trigram_map, const uint32_t*, size_t, uint16_t, trigram_match, uint32_t*, uint32_t*, void*) =
      blurrily_storage_find_references_device;
  uint32_t weight = 0, nb = 0;
  uint16_t codes[8];
  uint64_t offsets[2];
  int r = f_get(m, 1337u, &weight, 8, codes);
  r += f_get_batch(m, refs, 1, &weight, offsets, codes, 8);
  r += f_find(m, refs, 1, 10, rows, counts, &nb);
  r += f_find_dev(m, refs, 1, 10, rows, counts, NULL, NULL);
  return r;
}

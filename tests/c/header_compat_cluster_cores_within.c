/* header_compat_cluster_cores_within.c -- blurrily_storage_cluster_cores_within of include/blurrily_storage.h in ONE
 * translation unit with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by
 * tests/test_cluster_cores_within_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header
 * is never copied).  The reference has no clustering, so nothing of its own may clash with this prototype. */
#include "storage.h"
#include "blurrily_storage.h"

int cluster_cores_within_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* words, uint8_t* kinds);
int cluster_cores_within_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* words, uint8_t* kinds)
{
  int (*f_cores_within)(trigram_map, const uint32_t*, const uint32_t*, size_t, uint32_t, uint32_t, uint32_t*, uint32_t*,
                        uint8_t*, uint32_t*, uint64_t*, uint64_t*) =
      blurrily_storage_cluster_cores_within;
  uint32_t n_clusters = 0u;
  uint64_t n_edges = 0u, n_core_edges = 0u;
  /* refs: 4 references, then their 4 block keys; words: 4 labels, then 4 degrees */
  int r = f_cores_within(m, refs, refs + 4, 4, 700u, 3u, words, words + 4, kinds, &n_clusters, &n_edges, &n_core_edges);
  r += f_cores_within(m, refs, refs + 4, 4, 0u, 0u, words, NULL, NULL, NULL, NULL, NULL);
  r += f_cores_within(m, NULL, NULL, 0, 1000u, 0xFFFFFFFFu, NULL, NULL, NULL, NULL, NULL, NULL);
  r += (kinds[0] == BLURRILY_KIND_NONE) + (kinds[1] == BLURRILY_KIND_NOISE) + (kinds[2] == BLURRILY_KIND_BORDER) +
       (kinds[3] == BLURRILY_KIND_CORE);
  return r + (int)n_clusters + (int)n_edges + (int)n_core_edges + (words[0] == BLURRILY_NO_CLUSTER);
}

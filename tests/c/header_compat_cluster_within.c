/* header_compat_cluster_within.c -- blurrily_storage_cluster_within of include/blurrily_storage.h in ONE translation
 * unit with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by
 * tests/test_cluster_within_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is
 * never copied).  The reference has no clustering, so nothing of its own may clash with this prototype. */
#include "storage.h"
#include "blurrily_storage.h"

int cluster_within_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* words);
int cluster_within_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* words)
{
  int (*f_within)(trigram_map, const uint32_t*, const uint32_t*, size_t, uint32_t, uint32_t*, uint32_t*, uint64_t*) =
      blurrily_storage_cluster_within;
  uint32_t n_clusters = 0u;
  uint64_t n_edges = 0u;
  /* refs: 4 references, then their 4 block keys; words: 4 labels */
  int r = f_within(m, refs, refs + 4, 4, 700u, words, &n_clusters, &n_edges);
  r += f_within(m, refs, refs + 4, 4, 0u, words, NULL, NULL);
  r += f_within(m, NULL, NULL, 0, 1000u, NULL, NULL, NULL);
  return r + (int)n_clusters + (int)n_edges + (words[0] == BLURRILY_NO_CLUSTER);
}

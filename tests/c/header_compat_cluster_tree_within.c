/* header_compat_cluster_tree_within.c -- blurrily_storage_cluster_tree_within of include/blurrily_storage.h in ONE
 * translation unit with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by
 * tests/test_cluster_tree_within_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header
 * is never copied).  The reference has no clustering, so nothing of its own may clash with this prototype. */
#include "storage.h"
#include "blurrily_storage.h"

typedef char merge_record_is_three_words[sizeof(blurrily_cluster_merge_t) == 12 ? 1 : -1];

int cluster_tree_within_compat_calls(trigram_map m, const uint32_t* refs, const uint32_t* keys, uint32_t* words,
                                     blurrily_cluster_merge_t* merges);
int cluster_tree_within_compat_calls(trigram_map m, const uint32_t* refs, const uint32_t* keys, uint32_t* words,
                                     blurrily_cluster_merge_t* merges)
{
  int (*f_tree)(trigram_map, const uint32_t*, const uint32_t*, size_t, uint32_t, uint32_t*, blurrily_cluster_merge_t*,
                uint32_t*, uint32_t*, uint64_t*) = blurrily_storage_cluster_tree_within;
  uint32_t n_merges = 0u, n_clusters = 0u;
  uint64_t n_edges = 0u;
  /* refs: 4 references; keys: their 4 block keys; words: 4 labels; merges: room for 4 records */
  int r = f_tree(m, refs, keys, 4, 700u, words, merges, &n_merges, &n_clusters, &n_edges);
  r += f_tree(m, refs, keys, 4, 0u, words, merges, NULL, NULL, NULL);
  r += f_tree(m, NULL, NULL, 0, 1000u, NULL, NULL, NULL, NULL, NULL);
  if (n_merges && merges[0].a < merges[0].b) r += (int)merges[0].permille;
  return r + (int)n_merges + (int)n_clusters + (int)n_edges + (words[0] == BLURRILY_NO_CLUSTER) +
         (BLURRILY_CLUSTER_TREE_MAX == (1u << 27));
}

/* header_compat_cluster_core_tree_within.c -- blurrily_storage_cluster_core_tree_within of include/blurrily_storage.h in
 * ONE translation unit with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by
 * tests/test_cluster_core_tree_within_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the
 * header is never copied).  The reference has no clustering, so nothing of its own may clash with this prototype. */
#include "storage.h"
#include "blurrily_storage.h"

typedef char merge_record_is_three_words[sizeof(blurrily_cluster_merge_t) == 12 ? 1 : -1];

int cluster_core_tree_within_compat_calls(trigram_map m, const uint32_t* refs, const uint32_t* keys, uint32_t* words,
                                          uint32_t* heights, blurrily_cluster_merge_t* merges);
int cluster_core_tree_within_compat_calls(trigram_map m, const uint32_t* refs, const uint32_t* keys, uint32_t* words,
                                          uint32_t* heights, blurrily_cluster_merge_t* merges)
{
  int (*f_tree)(trigram_map, const uint32_t*, const uint32_t*, size_t, uint32_t, uint32_t, uint32_t*, uint32_t*,
                blurrily_cluster_merge_t*, uint32_t*, uint32_t*, uint64_t*, uint64_t*) =
      blurrily_storage_cluster_core_tree_within;
  uint32_t n_merges = 0u, n_clusters = 0u;
  uint64_t n_edges = 0u, n_core_edges = 0u;
  /* refs: 4 references; keys: their 4 block keys; words: 4 labels; heights: 4 core heights; merges: room for 4 records */
  int r = f_tree(m, refs, keys, 4, 700u, 3u, words, heights, merges, &n_merges, &n_clusters, &n_edges, &n_core_edges);
  r += f_tree(m, refs, keys, 4, 0u, 0u, words, heights, merges, NULL, NULL, NULL, NULL);
  r += f_tree(m, NULL, NULL, 0, 1000u, 0xFFFFFFFFu, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  if (n_merges && merges[0].a < merges[0].b) r += (int)merges[0].permille;
  return r + (int)n_merges + (int)n_clusters + (int)n_edges + (int)n_core_edges + (words[0] == BLURRILY_NO_CLUSTER) +
         (heights[0] == BLURRILY_NO_CORE) + (BLURRILY_CLUSTER_TREE_MAX == (1u << 27));
}

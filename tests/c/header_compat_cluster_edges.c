/* header_compat_cluster_edges.c -- blurrily_storage_cluster_edges and blurrily_storage_cluster_edges_within of
 * include/blurrily_storage.h in ONE translation unit with the reference's ext/blurrily/storage.h, compiled with
 * -std=c99 -Wall -Wextra -Werror by tests/test_cluster_edges_abi.py.  "storage.h" is the stand-in made from
 * tests/golden/ref_abi.json (the header is never copied).  The reference has no clustering, so nothing of its own may
 * clash with these prototypes. */
#include "storage.h"
#include "blurrily_storage.h"

typedef char edge_record_is_three_words[sizeof(blurrily_cluster_merge_t) == 12 ? 1 : -1];

int cluster_edges_compat_calls(trigram_map m, const uint32_t* refs, const uint32_t* keys,
                               blurrily_cluster_merge_t* edges);
int cluster_edges_compat_calls(trigram_map m, const uint32_t* refs, const uint32_t* keys,
                               blurrily_cluster_merge_t* edges)
{
  int (*f_edges)(trigram_map, const uint32_t*, size_t, uint32_t, blurrily_cluster_merge_t*, uint64_t,
                 uint64_t*) = blurrily_storage_cluster_edges;
  int (*f_within)(trigram_map, const uint32_t*, const uint32_t*, size_t, uint32_t, blurrily_cluster_merge_t*, uint64_t,
                  uint64_t*) = blurrily_storage_cluster_edges_within;
  uint64_t n_edges = 0u, n_within = 0u;
  /* refs: 4 references; keys: their 4 block keys; edges: room for 6 records */
  int r = f_edges(m, refs, 4, 700u, NULL, 0u, &n_edges);       /* count only */
  r += f_edges(m, refs, 4, 700u, edges, 6u, &n_edges);
  r += f_edges(m, NULL, 0, 1000u, NULL, 0u, &n_edges);
  r += f_within(m, refs, keys, 4, 700u, NULL, 0u, &n_within);
  r += f_within(m, refs, keys, 4, 0u, edges, 6u, &n_within);
  r += f_within(m, NULL, NULL, 0, 1000u, edges, 6u, &n_within);
  if (n_edges && edges[0].a < edges[0].b) r += (int)edges[0].permille;
  return r + (int)n_edges + (int)n_within + (BLURRILY_CLUSTER_TREE_MAX == (1u << 27));
}

/* header_compat_cluster_edges_extend.c -- blurrily_storage_cluster_edges_extend and
 * blurrily_storage_cluster_edges_between of include/blurrily_storage.h in ONE translation unit with the reference's
 * ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by tests/test_cluster_edges_extend_abi.py.
 * "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is never copied).  The reference has no
 * clustering, so nothing of its own may clash with these prototypes. */
#include "storage.h"
#include "blurrily_storage.h"

typedef char edge_record_is_three_words[sizeof(blurrily_cluster_merge_t) == 12 ? 1 : -1];

int cluster_edges_extend_compat_calls(trigram_map m, const uint32_t* first, const uint32_t* second,
                                      blurrily_cluster_merge_t* edges);
int cluster_edges_extend_compat_calls(trigram_map m, const uint32_t* first, const uint32_t* second,
                                      blurrily_cluster_merge_t* edges)
{
  int (*f_extend)(trigram_map, const uint32_t*, size_t, const uint32_t*, size_t, uint32_t,
                  blurrily_cluster_merge_t*, uint64_t, uint64_t*) = blurrily_storage_cluster_edges_extend;
  int (*f_between)(trigram_map, const uint32_t*, size_t, const uint32_t*, size_t, uint32_t,
                   blurrily_cluster_merge_t*, uint64_t, uint64_t*) = blurrily_storage_cluster_edges_between;
  uint64_t n_extend = 0u, n_between = 0u;
  /* first: 4 references; second: 2 references; edges: room for 9 records */
  int r = f_extend(m, first, 4, second, 2, 700u, NULL, 0u, &n_extend);   /* count only */
  r += f_extend(m, first, 4, second, 2, 700u, edges, 9u, &n_extend);
  r += f_extend(m, NULL, 0, second, 2, 1000u, edges, 9u, &n_extend);
  r += f_extend(m, first, 4, NULL, 0, 0u, NULL, 0u, &n_extend);
  r += f_between(m, first, 4, second, 2, 700u, NULL, 0u, &n_between);
  r += f_between(m, second, 2, first, 4, 700u, edges, 9u, &n_between);
  r += f_between(m, NULL, 0, NULL, 0, 1000u, edges, 9u, &n_between);
  if (n_extend && edges[0].a < edges[0].b) r += (int)edges[0].permille;
  return r + (int)n_extend + (int)n_between + (BLURRILY_CLUSTER_TREE_MAX == (1u << 27));
}

/* header_compat_cluster.c -- blurrily_storage_cluster of include/blurrily_storage.h in ONE translation unit with the
 * reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by tests/test_cluster_abi.py.
 * "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is never copied).  The reference has no
 * clustering, so nothing of its own may clash with this prototype. */
#include "storage.h"
#include "blurrily_storage.h"

int cluster_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* labels);
int cluster_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* labels)
{
  int (*f_cluster)(trigram_map, const uint32_t*, size_t, uint32_t, uint32_t*, uint32_t*, uint64_t*) =
      blurrily_storage_cluster;
  uint32_t n_clusters = 0u;
  uint64_t n_edges = 0u;
  int r = f_cluster(m, refs, 4, 700u, labels, &n_clusters, &n_edges);
  r += f_cluster(m, refs, 4, 0u, labels, NULL, NULL);
  return r + (int)n_clusters + (int)n_edges + (labels[0] == BLURRILY_NO_CLUSTER);
}

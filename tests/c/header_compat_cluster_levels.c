/* header_compat_cluster_levels.c -- blurrily_storage_cluster_levels of include/blurrily_storage.h in ONE translation
 * unit with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by
 * tests/test_cluster_levels_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is
 * never copied).  The reference has no clustering, so nothing of its own may clash with this prototype. */
#include "storage.h"
#include "blurrily_storage.h"

int cluster_levels_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* labels);
int cluster_levels_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* labels)
{
  int (*f_levels)(trigram_map, const uint32_t*, size_t, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint64_t*) =
      blurrily_storage_cluster_levels;
  const uint32_t floors[3] = {500u, 700u, 900u};
  uint32_t n_clusters[BLURRILY_CLUSTER_MAX_LEVELS] = {0u};
  uint64_t n_edges[BLURRILY_CLUSTER_MAX_LEVELS] = {0u};
  int r = f_levels(m, refs, 4, floors, 3u, labels, n_clusters, n_edges);   /* labels: 3 * 4 words */
  r += f_levels(m, refs, 4, floors, 1u, labels, NULL, NULL);
  return r + (int)n_clusters[2] + (int)n_edges[2] + (labels[2 * 4] == BLURRILY_NO_CLUSTER);
}

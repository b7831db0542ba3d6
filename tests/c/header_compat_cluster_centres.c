/* header_compat_cluster_centres.c -- blurrily_storage_cluster_centres of include/blurrily_storage.h in ONE translation
 * unit with the reference's ext/blurrily/storage.h, compiled with -std=c99 -Wall -Wextra -Werror by
 * tests/test_cluster_centres_abi.py.  "storage.h" is the stand-in made from tests/golden/ref_abi.json (the header is
 * never copied).  The reference has no clustering, so nothing of its own may clash with this prototype. */
#include "storage.h"
#include "blurrily_storage.h"

int cluster_centres_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* words, uint8_t* attached);
int cluster_centres_compat_calls(trigram_map m, const uint32_t* refs, uint32_t* words, uint8_t* attached)
{
  int (*f_centres)(trigram_map, const uint32_t*, size_t, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint8_t*,
                   uint32_t*, uint64_t*) =
      blurrily_storage_cluster_centres;
  uint32_t n_clusters = 0u;
  uint64_t n_edges = 0u;
  int r = f_centres(m, refs, 4, 700u, words, words + 4, words + 8, attached, &n_clusters, &n_edges);   /* words: 3 * 4 */
  r += f_centres(m, refs, 4, 0u, words, NULL, NULL, NULL, NULL, NULL);
  return r + (int)n_clusters + (int)n_edges + (words[8] == BLURRILY_NO_CLUSTER) + attached[0];
}

// The host clique header (guacamole_amd/csrc/gq_sv_clique.h) as a stand-alone program
// (tests/test_structural_variant.py).  stdin: the number of cases, then per case
//   N n m
//   n lines: contig lo hi len        (nodes in (contig, lo) order)
//   m lines: i j weight              (edges, i < j)
// stdout per case: the number of cliques, then one line each: contig start stop pairs wiggle.
#include <cstdio>
#include <vector>

#include "../../guacamole_amd/csrc/gq_sv_clique.h"

int main() {
  long long cases = 0;
  if (scanf("%lld", &cases) != 1) return 2;
  for (long long c = 0; c < cases; ++c) {
    long long N, n, m;
    if (scanf("%lld %lld %lld", &N, &n, &m) != 3 || n < 0 || m < 0) return 2;
    std::vector<int32_t> contig((size_t)n), lo((size_t)n), hi((size_t)n), len((size_t)n), ei((size_t)m), ej((size_t)m);
    std::vector<int64_t> w((size_t)m);
    for (long long k = 0; k < n; ++k)
      if (scanf("%d %d %d %d", &contig[(size_t)k], &lo[(size_t)k], &hi[(size_t)k], &len[(size_t)k]) != 4) return 2;
    for (long long k = 0; k < m; ++k) {
      long long x;
      if (scanf("%d %d %lld", &ei[(size_t)k], &ej[(size_t)k], &x) != 3) return 2;
      if (ei[(size_t)k] < 0 || ej[(size_t)k] <= ei[(size_t)k] || ej[(size_t)k] >= n) return 3;
      w[(size_t)k] = x;
    }
    const std::vector<gq_sv::Clique> got =
        gq_sv::find_cliques(n, contig.data(), lo.data(), hi.data(), len.data(), m, ei.data(), ej.data(), w.data(), N);
    printf("%zu\n", got.size());
    for (const gq_sv::Clique &q : got)
      printf("%d %lld %lld %lld %lld\n", q.contig, (long long)q.start, (long long)q.stop, (long long)q.pairs,
             (long long)q.wiggle);
  }
  return 0;
}

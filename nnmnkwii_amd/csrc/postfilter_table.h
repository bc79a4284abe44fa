// The table of the Merlin post-filter (K8, postfilter.hip): G (fftlen/2 + 1, D) row-major float64 with
//   Re DFT_fftlen(freqt(c, order, -alpha))[k] = sum_d G[k][d] c[d].
// Host code without HIP: a stand-alone program can compile it with any C++ compiler (that is how it is run under the address and
// undefined-behaviour sanitizers).  G = C A with A[:, d] = freqt(e_d, order, -alpha), the literal recursion of the published SPTK
// algorithm on the unit vectors, and C[k][j] = cos(2 pi (k j mod fftlen) / fftlen): the phase is reduced as an integer and looked
// up in a table of fftlen roots (the discipline of modspec_dft.hip), the sum over j runs upwards.
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

namespace mlpg {

constexpr int kPfMaxD = 64, kPfMinFft = 4, kPfMaxFft = 4096;

// 0, or the 1-based index of the first limit that fails: 1 D, 2 fftlen, 3 order, 4 alpha
inline int postfilter_check_limits(int D, double alpha, int order, int fftlen) {
  if (D < 1 || D > kPfMaxD) return 1;
  if (fftlen < kPfMinFft || fftlen > kPfMaxFft || (fftlen & (fftlen - 1))) return 2;
  if (order < D - 1 || order >= fftlen) return 3;
  if (!(fabs(alpha) < 1.0)) return 4;
  return 0;
}

// freqt(c1[0 .. m1], m2, a) -> g[0 .. m2]; d is scratch of m2 + 1 doubles
inline void postfilter_freqt(const double *c1, int m1, int m2, double a, double *g, double *d) {
  const double beta = 1.0 - a * a;
  for (int j = 0; j <= m2; ++j) g[j] = d[j] = 0.0;
  for (int i = -m1; i <= 0; ++i) {
    for (int j = 0; j <= m2; ++j) d[j] = g[j];
    g[0] = c1[-i] + a * d[0];
    if (m2 >= 1) g[1] = beta * d[0] + a * d[1];
    for (int j = 2; j <= m2; ++j) g[j] = d[j - 1] + a * (d[j] - g[j - 1]);
  }
}

// Returns postfilter_check_limits' answer (nothing is written unless it is 0).
inline int postfilter_table(int D, double alpha, int order, int fftlen, double *G) {
  if (int rc = postfilter_check_limits(D, alpha, order, fftlen)) return rc;
  const int m2 = order, N = fftlen, bins = N / 2 + 1;
  std::vector<double> A((size_t)(m2 + 1) * D), g(m2 + 1), d(m2 + 1), e(D), roots(N);
  for (int c = 0; c < D; ++c) {
    for (int i = 0; i <= c; ++i) e[i] = i == c ? 1.0 : 0.0;
    postfilter_freqt(e.data(), c, m2, -alpha, g.data(), d.data());
    for (int j = 0; j <= m2; ++j) A[(size_t)j * D + c] = g[j];
  }
  const long double two_pi = 6.283185307179586476925286766559L;
  for (int p = 0; p < N; ++p) roots[p] = (double)cosl(two_pi * (long double)p / (long double)N);
  roots[0] = 1.0;
  roots[N / 2] = -1.0;
  roots[N / 4] = roots[3 * (N / 4)] = 0.0;
  for (int k = 0; k < bins; ++k) {
    double *row = G + (size_t)k * D;
    for (int c = 0; c < D; ++c) row[c] = 0.0;
    for (int j = 0; j <= m2; ++j) {
      const double w = roots[(int)(((long)k * j) % N)];
      const double *a = A.data() + (size_t)j * D;
      for (int c = 0; c < D; ++c) row[c] += w * a[c];
    }
  }
  return 0;
}

}  // namespace mlpg

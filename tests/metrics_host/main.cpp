// Stand-alone driver of the host build of csrc/frame_metrics.hip (tests/test_metrics_host_cpu.py): metrics_host in.bin out.bin.
// in.bin: int64 B, Tmax, ld_x, ld_y, dtype_x, dtype_y, has_lengths, nterms, want_per_utt; int32 lengths[B]; x[B Tmax ld_x] of
// dtype_x; y[B Tmax ld_y] of dtype_y; nnmk_metrics_term terms[nterms].
// out.bin: double totals[nterms 2]; double per_utt[B nterms 2] if want_per_utt; then the workspace (the partials).
// Every array is an exact-size heap block (ASan), the workspace exactly nnmk_metrics_workspace bytes.
#include "extras.h"
#include "csrc/x/frame_metrics_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[9];
  f.read((char *)h, sizeof h);
  const int B = (int)h[0], Tmax = (int)h[1], nterms = (int)h[7];
  auto len = rd<int32_t>(f, B);
  auto x = rd<char>(f, (size_t)B * Tmax * h[2] * (h[4] ? 8 : 4));
  auto y = rd<char>(f, (size_t)B * Tmax * h[3] * (h[5] ? 8 : 4));
  auto terms = rd<nnmk_metrics_term>(f, nterms);
  const int64_t bytes = nnmk_metrics_workspace(B, Tmax, nterms);
  if (bytes < 0) return 3;
  std::vector<double> ws((size_t)bytes / 8, -7.0), totals(2 * (size_t)nterms, -7.0), per(h[8] ? 2 * (size_t)nterms * B : 0, -7.0);
  const int rc = nnmk_metrics_batch(0, nullptr, (int)h[4], x.data(), h[2], (int)h[5], y.data(), h[3], h[6] ? len.data() : nullptr, B, Tmax,
                                    terms.data(), nterms, h[8] ? per.data() : nullptr, totals.data(), ws.data(), bytes);
  if (rc) { fprintf(stderr, "nnmk_metrics_batch rc %d\n", rc); return 1; }
  if (nnmk_metrics_launch_count() != 1) return 4;
  std::ofstream o(argv[2], std::ios::binary);
  o.write((const char *)totals.data(), totals.size() * 8);
  o.write((const char *)per.data(), per.size() * 8);
  o.write((const char *)ws.data(), ws.size() * 8);
  return 0;
}

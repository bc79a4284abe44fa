// Stand-alone driver of the host build of csrc/postfilter.hip (tests/test_postfilter_host_cpu.py): postfilter_host in.bin out.bin.
// in.bin: int64 B, Tmax, D, ld_in, ld_out, dtype, has_lengths, in_place, fftlen, order; double alpha; int32 lengths[B];
// mgc[B Tmax ld_in] of dtype; double weight[D].  The table G (fftlen/2 + 1, D) is built here by mlpg_hip_postfilter_table.
// out.bin: out[B Tmax ld_out] of dtype (prefilled with -7), or mgc itself after the call in place.
// Every array is an exact-size heap block (ASan).
#include "extras.h"
#include "csrc/x/postfilter_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
template <typename T>
static int run(std::ifstream &f, const int64_t *h, double alpha, const char *out_path) {
  const int B = (int)h[0], Tmax = (int)h[1], D = (int)h[2], fftlen = (int)h[8];
  auto len = rd<int32_t>(f, B);
  auto x = rd<T>(f, (size_t)B * Tmax * h[3]);
  auto w = rd<double>(f, D);
  std::vector<double> G((size_t)(fftlen / 2 + 1) * D);
  int rc = mlpg_hip_postfilter_table(D, alpha, (int)h[9], fftlen, G.data());
  if (rc) { fprintf(stderr, "postfilter_table rc %d\n", rc); return 1; }
  std::vector<T> y(h[7] ? 0 : (size_t)B * Tmax * h[4], (T)-7);
  T *out = h[7] ? x.data() : y.data();
  rc = mlpg_hip_merlin_post_filter(0, nullptr, (int)h[5], x.data(), h[3], h[6] ? len.data() : nullptr, B, Tmax, D, alpha, w.data(), G.data(),
                                   fftlen, out, h[7] ? h[3] : h[4]);
  if (rc) { fprintf(stderr, "merlin_post_filter rc %d\n", rc); return 1; }
  std::ofstream o(out_path, std::ios::binary);
  o.write((const char *)out, (h[7] ? x.size() : y.size()) * sizeof(T));
  return 0;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[10];
  double alpha;
  f.read((char *)h, sizeof h);
  f.read((char *)&alpha, 8);
  return h[5] == 0 ? run<float>(f, h, alpha, argv[2]) : run<double>(f, h, alpha, argv[2]);
}

// Stand-alone driver of the host build of csrc/modspec_filter.hip (tests/test_msfilter_host_cpu.py): msfilter_host in.bin out.bin.
// in.bin: int64 B, T, D, n, ld_x, ld_out, dtype, has_lengths, has_tables, limit_bin, log_domain, ortho, in_place; int32
// lengths[B]; x[B T ld_x] of dtype; double A[(n/2+1) D], C[(n/2+1) D] if has_tables.
// out.bin: out[B T ld_out] of dtype (prefilled with -7), or x itself after the call in place.
// Every array is an exact-size heap block (ASan); so is the dynamic LDS of every launch (the shim).
#include "extras.h"
#include "csrc/x/modspec_filter_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
template <typename TX>
static int run(std::ifstream &f, const int64_t *h, const char *out_path) {
  const int B = (int)h[0], T = (int)h[1], D = (int)h[2], n = (int)h[3];
  auto len = rd<int32_t>(f, B);
  auto x = rd<TX>(f, (size_t)B * T * h[4]);
  const size_t nt = h[8] ? (size_t)(n / 2 + 1) * D : 0;
  auto A = rd<double>(f, nt), C = rd<double>(f, nt);
  std::vector<TX> y(h[12] ? 0 : (size_t)B * T * h[5], (TX)-7);
  TX *out = h[12] ? x.data() : y.data();
  const int rc = mlpg_hip_modspec_filter(0, nullptr, (int)h[6], x.data(), h[4], h[7] ? len.data() : nullptr, B, T, D, n, (int)h[11],
                                         h[8] ? A.data() : nullptr, h[8] ? C.data() : nullptr, (int)h[9], (int)h[10], out,
                                         h[12] ? h[4] : h[5]);
  if (rc) { fprintf(stderr, "modspec_filter rc %d\n", rc); return 1; }
  std::ofstream o(out_path, std::ios::binary);
  o.write((const char *)out, (h[12] ? x.size() : y.size()) * sizeof(TX));
  return 0;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[13];
  f.read((char *)h, sizeof h);
  return h[6] == 0 ? run<float>(f, h, argv[2]) : run<double>(f, h, argv[2]);
}

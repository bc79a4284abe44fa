// Stand-alone driver of the host build of csrc/colstats.hip (tests/test_norm_host_cpu.py): norm_host in.bin out.bin.
// in.bin: int64 op, B, Tmax, D, ld_x, in_dtype, has_lengths, has_state, in_place, out_dtype, ld_y, mode; int32 lengths[B];
// x[B Tmax ld_x] of in_dtype; then op 0 (statistics): double state_in[5 D] if has_state; op 1 (apply): double a[D], c[D].
// out.bin, op 0: double state_out[5 D], then the workspace (the partials); op 1: y[B Tmax ld_y] of out_dtype (prefilled with -7).
// Every array is an exact-size heap block (ASan), the workspace exactly mlpg_hip_column_stats_workspace bytes.
#include "extras.h"
#include "colstats_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
template <typename TX>
static int run(std::ifstream &f, const int64_t *h, const char *out_path) {
  const int op = (int)h[0], B = (int)h[1], Tmax = (int)h[2], D = (int)h[3];
  const int64_t ld_x = h[4], ld_y = h[10];
  auto len = rd<int32_t>(f, B);
  auto x = rd<TX>(f, (size_t)B * Tmax * ld_x);
  const int32_t *lp = h[6] ? len.data() : nullptr;
  std::ofstream o(out_path, std::ios::binary);
  if (op == 0) {
    auto st = rd<double>(f, h[7] ? 5 * (size_t)D : 0);
    std::vector<double> out(5 * (size_t)D, -7.0);
    if (h[8]) out = st;   // in place: state_out is state_in
    const int64_t bytes = mlpg_hip_column_stats_workspace(B, Tmax, D);
    if (bytes < 0) return 3;
    std::vector<double> ws((size_t)bytes / 8, -7.0);
    const int rc = mlpg_hip_column_stats(0, nullptr, (int)h[5], x.data(), ld_x, lp, B, Tmax, D, h[7] ? (h[8] ? out.data() : st.data()) : nullptr,
                                         out.data(), ws.data(), bytes);
    if (rc) { fprintf(stderr, "column_stats rc %d\n", rc); return 1; }
    o.write((const char *)out.data(), out.size() * 8);
    o.write((const char *)ws.data(), ws.size() * 8);
    return 0;
  }
  auto a = rd<double>(f, D), c = rd<double>(f, D);
  int rc;
  if (h[8]) {
    rc = mlpg_hip_column_affine(0, nullptr, (int)h[5], (int)h[5], (int)h[11], x.data(), ld_x, x.data(), ld_x, lp, B, Tmax, D, a.data(), c.data());
    o.write((const char *)x.data(), x.size() * sizeof(TX));
  } else if (h[9] == 0) {
    std::vector<float> y((size_t)B * Tmax * ld_y, -7.0f);
    rc = mlpg_hip_column_affine(0, nullptr, (int)h[5], 0, (int)h[11], x.data(), ld_x, y.data(), ld_y, lp, B, Tmax, D, a.data(), c.data());
    o.write((const char *)y.data(), y.size() * 4);
  } else {
    std::vector<double> y((size_t)B * Tmax * ld_y, -7.0);
    rc = mlpg_hip_column_affine(0, nullptr, (int)h[5], 1, (int)h[11], x.data(), ld_x, y.data(), ld_y, lp, B, Tmax, D, a.data(), c.data());
    o.write((const char *)y.data(), y.size() * 8);
  }
  if (rc) { fprintf(stderr, "column_affine rc %d\n", rc); return 1; }
  return 0;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[12];
  f.read((char *)h, sizeof h);
  return h[5] == 0 ? run<float>(f, h, argv[2]) : run<double>(f, h, argv[2]);
}

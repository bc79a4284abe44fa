// Stand-alone driver of the host build of csrc/mlpg_gv.hip (tests/test_gvmlpg_host_cpu.py): gvmlpg_host in.bin out.bin.
// in.bin: int64 B, Tmax, D, nw, dtype, var_mode, has_lengths, n_iter, init, in_place; double omega_scale, step; int32 lengths[B],
// wl[nw], wu[nw]; double coef[sum (l + u + 1)]; then in `dtype` mean[B Tmax D], var[B Tmax D | D | 0], y_in[B Tmax sd]; double
// gv_mean[sd], gv_prec[sd].  out.bin: y_out[B Tmax sd] in `dtype` (prefilled with -7), double report[B sd 4], int32 status[B sd],
// double gv[B sd] (mlpg_hip_gv of y_out).  Every array is an exact-size heap block (ASan).
#include "extras.h"
#include "mlpg_gv_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
template <typename T>
static int run(std::ifstream &f, const int64_t *h, double omega_scale, double step, const char *out_path) {
  const int B = (int)h[0], Tmax = (int)h[1], D = (int)h[2], nw = (int)h[3], dtype = (int)h[4], var_mode = (int)h[5];
  const int sd = D / nw;
  auto len = rd<int32_t>(f, B), wl = rd<int32_t>(f, nw), wu = rd<int32_t>(f, nw);
  size_t nc = 0;
  for (int w = 0; w < nw; ++w) nc += wl[w] + wu[w] + 1;
  auto coef = rd<double>(f, nc);
  const size_t rows = (size_t)B * Tmax;
  auto mean = rd<T>(f, rows * D);
  auto var = rd<T>(f, var_mode == 0 ? rows * D : var_mode == 1 ? D : 0);
  auto y_in = rd<T>(f, rows * sd);
  auto gm = rd<double>(f, sd), gp = rd<double>(f, sd);
  std::vector<T> y_out(rows * sd, (T)-7);
  std::vector<double> report((size_t)B * sd * 4, -7.0), gv((size_t)B * sd, -7.0);
  std::vector<int32_t> status((size_t)B * sd, -7);
  T *yo = h[9] ? y_in.data() : y_out.data();
  int rc = mlpg_hip_gv_ascent(0, nullptr, dtype, mean.data(), var_mode == 2 ? nullptr : var.data(), var_mode, h[6] ? len.data() : nullptr, B,
                              Tmax, D, nw, wl.data(), wu.data(), coef.data(), y_in.data(), yo, gm.data(), gp.data(), omega_scale,
                              (int)h[7], step, (int)h[8], report.data(), status.data());
  if (rc) { fprintf(stderr, "gv_ascent rc %d\n", rc); return 1; }
  rc = mlpg_hip_gv(0, nullptr, dtype, yo, sd, h[6] ? len.data() : nullptr, B, Tmax, sd, gv.data());
  if (rc) { fprintf(stderr, "gv rc %d\n", rc); return 1; }
  std::ofstream o(out_path, std::ios::binary);
  o.write((const char *)yo, rows * sd * sizeof(T));
  o.write((const char *)report.data(), report.size() * 8);
  o.write((const char *)status.data(), status.size() * 4);
  o.write((const char *)gv.data(), gv.size() * 8);
  return 0;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[10];
  double s[2];
  f.read((char *)h, sizeof h);
  f.read((char *)s, sizeof s);
  return h[4] == 0 ? run<float>(f, h, s[0], s[1], argv[2]) : run<double>(f, h, s[0], s[1], argv[2]);
}

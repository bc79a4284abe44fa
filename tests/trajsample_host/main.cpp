// Stand-alone driver of the host build of csrc/mlpg_trajsample.hip (tests/test_trajsample_host_cpu.py): trajsample_host in.bin out.bin.
// in.bin: int64 B, Tmax, sd, nw, dtype, var_mode, has_lengths, K, has_mean, ld_in, ld_fac, ld_noise, ld_mean, ld_out, ld_z, Q;
// int32 lengths[B], wl[nw], wu[nw]; double coef[sum (l + u + 1)]; then in `dtype` var[span(B Tmax, ld_in, D) | D | 0],
// noise[span(K B Tmax, ld_noise, sd)], mean[span(B Tmax, ld_mean, sd)] if has_mean, where span(rows, ld, width) =
// (rows - 1) ld + width elements: every array is an exact-size heap block (ASan).
// out.bin: double factor[span((Q + 1) B Tmax, ld_fac, sd)], double logdet[B sd], int32 status[B sd], then in `dtype`
// out[span(K B Tmax, ld_out, sd)] and z[span(K B Tmax, ld_z, sd)] (all prefilled with -7).  The draws are made from the factor and
// status the factor call wrote; z is nnmk_draw_whiten of those draws.
#include "extras.h"
#include "csrc/x/mlpg_trajsample_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
static size_t span(size_t rows, size_t ld, size_t width) { return rows && width ? (rows - 1) * ld + width : 0; }
template <typename T>
static int run(std::ifstream &f, const int64_t *h, const char *out_path) {
  const int B = (int)h[0], Tmax = (int)h[1], sd = (int)h[2], nw = (int)h[3], dtype = (int)h[4], var_mode = (int)h[5], K = (int)h[7], Q = (int)h[15];
  const int D = nw * sd;
  const int64_t ld_in = h[9], ld_fac = h[10], ld_noise = h[11], ld_mean = h[12], ld_out = h[13], ld_z = h[14];
  auto len = rd<int32_t>(f, B), wl = rd<int32_t>(f, nw), wu = rd<int32_t>(f, nw);
  size_t nc = 0;
  for (int w = 0; w < nw; ++w) nc += wl[w] + wu[w] + 1;
  auto coef = rd<double>(f, nc);
  const size_t rows = (size_t)B * Tmax;
  auto var = rd<T>(f, var_mode == 0 ? span(rows, ld_in, D) : var_mode == 1 ? D : 0);
  auto noise = rd<T>(f, span((size_t)K * rows, ld_noise, sd));
  auto mean = rd<T>(f, h[8] ? span(rows, ld_mean, sd) : 0);
  std::vector<double> fac(span((size_t)(Q + 1) * rows, ld_fac, sd), -7.0), logdet((size_t)B * sd, -7.0);
  std::vector<int32_t> status((size_t)B * sd, -7);
  std::vector<T> out(span((size_t)K * rows, ld_out, sd), (T)-7), z(span((size_t)K * rows, ld_z, sd), (T)-7);
  const int32_t *lp = h[6] ? len.data() : nullptr;
  const void *vp = var_mode == 2 ? nullptr : (const void *)var.data();
  const void *mp = h[8] ? (const void *)mean.data() : nullptr;
  int rc = nnmk_draw_factor(0, nullptr, dtype, vp, var_mode, ld_in, lp, B, Tmax, D, sd, nw, wl.data(), wu.data(), coef.data(), fac.data(), ld_fac,
                            logdet.data(), status.data());
  if (rc) { fprintf(stderr, "factor rc %d\n", rc); return 1; }
  rc = nnmk_draw_sample(0, nullptr, dtype, fac.data(), ld_fac, status.data(), lp, B, Tmax, sd, Q, K, noise.data(), ld_noise, mp, ld_mean, out.data(),
                        ld_out);
  if (rc) { fprintf(stderr, "sample rc %d\n", rc); return 1; }
  rc = nnmk_draw_whiten(0, nullptr, dtype, fac.data(), ld_fac, status.data(), lp, B, Tmax, sd, Q, K, out.data(), ld_out, mp, ld_mean, z.data(), ld_z);
  if (rc) { fprintf(stderr, "whiten rc %d\n", rc); return 1; }
  std::ofstream o(out_path, std::ios::binary);
  o.write((const char *)fac.data(), fac.size() * 8);
  o.write((const char *)logdet.data(), logdet.size() * 8);
  o.write((const char *)status.data(), status.size() * 4);
  o.write((const char *)out.data(), out.size() * sizeof(T));
  o.write((const char *)z.data(), z.size() * sizeof(T));
  return 0;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[16];
  f.read((char *)h, sizeof h);
  return h[4] == 0 ? run<float>(f, h, argv[2]) : run<double>(f, h, argv[2]);
}

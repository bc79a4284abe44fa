// Stand-alone driver of the host build of csrc/mlpg_trajcov.hip (tests/test_trajcov_host_cpu.py): trajcov_host in.bin out.bin.
// in.bin: int64 B, Tmax, sd, nw, dtype, var_mode, has_lengths, want_band, do_nll, want_gm, want_gv, ld_in, ld_band, ld_cbar,
// ld_target, Q; int32 lengths[B], wl[nw], wu[nw]; double coef[sum (l + u + 1)]; then in `dtype` var[span(B Tmax, ld_in, D) | D | 0]
// and, if do_nll, mean[span(B Tmax, ld_in, D)], cbar[span(B Tmax, ld_cbar, sd)], target[span(B Tmax, ld_target, sd)], where
// span(rows, ld, width) = (rows - 1) ld + width elements: every array is an exact-size heap block (ASan).
// out.bin: double band[span((Q + 1) B Tmax, ld_band, sd)] (prefilled with -7; absent without want_band), double logdet[B sd],
// int32 status[B sd]; if do_nll: double nll[B sd], then in `dtype` gm[B Tmax D] if want_gm, gv[B Tmax D | D] if want_gv (all
// prefilled with -7).  The likelihood is called with the band and logdet the covariance call wrote.
#include "extras.h"
#include "csrc/x/mlpg_trajcov_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
static size_t span(size_t rows, size_t ld, size_t width) { return rows && width ? (rows - 1) * ld + width : 0; }
template <typename T>
static int run(std::ifstream &f, const int64_t *h, const char *out_path) {
  const int B = (int)h[0], Tmax = (int)h[1], sd = (int)h[2], nw = (int)h[3], dtype = (int)h[4], var_mode = (int)h[5], Q = (int)h[15];
  const int D = nw * sd;
  const int64_t ld_in = h[11], ld_band = h[12], ld_cbar = h[13], ld_target = h[14];
  auto len = rd<int32_t>(f, B), wl = rd<int32_t>(f, nw), wu = rd<int32_t>(f, nw);
  size_t nc = 0;
  for (int w = 0; w < nw; ++w) nc += wl[w] + wu[w] + 1;
  auto coef = rd<double>(f, nc);
  const size_t rows = (size_t)B * Tmax;
  auto var = rd<T>(f, var_mode == 0 ? span(rows, ld_in, D) : var_mode == 1 ? D : 0);
  std::vector<double> band(h[7] ? span((size_t)(Q + 1) * rows, ld_band, sd) : 0, -7.0), logdet((size_t)B * sd, -7.0);
  std::vector<int32_t> status((size_t)B * sd, -7);
  const int32_t *lp = h[6] ? len.data() : nullptr;
  const void *vp = var_mode == 2 ? nullptr : (const void *)var.data();
  int rc = nnmk_traj_covariance(0, nullptr, dtype, vp, var_mode, ld_in, lp, B, Tmax, D, sd, nw, wl.data(), wu.data(), coef.data(),
                                (int)h[7], h[7] ? band.data() : nullptr, ld_band, logdet.data(), status.data());
  if (rc) { fprintf(stderr, "covariance rc %d\n", rc); return 1; }
  std::ofstream o(out_path, std::ios::binary);
  o.write((const char *)band.data(), band.size() * 8);
  o.write((const char *)logdet.data(), logdet.size() * 8);
  o.write((const char *)status.data(), status.size() * 4);
  if (h[8]) {
    auto mean = rd<T>(f, span(rows, ld_in, D)), cbar = rd<T>(f, span(rows, ld_cbar, sd)), target = rd<T>(f, span(rows, ld_target, sd));
    std::vector<double> nll((size_t)B * sd, -7.0);
    std::vector<T> gm(h[9] ? rows * D : 0, (T)-7), gv(h[10] ? (var_mode == 0 ? rows * D : D) : 0, (T)-7);
    const int64_t need = nnmk_traj_nll_workspace(var_mode, (int)h[10], B, D);
    std::vector<double> work((size_t)need / 8, -7.0);
    rc = nnmk_traj_nll(0, nullptr, dtype, mean.data(), vp, var_mode, ld_in, lp, B, Tmax, D, sd, nw, wl.data(), wu.data(), coef.data(),
                       cbar.data(), ld_cbar, target.data(), ld_target, h[7] ? band.data() : nullptr, ld_band, logdet.data(), nll.data(),
                       h[9] ? gm.data() : nullptr, h[10] ? gv.data() : nullptr, need ? work.data() : nullptr, need);
    if (rc) { fprintf(stderr, "nll rc %d\n", rc); return 1; }
    o.write((const char *)nll.data(), nll.size() * 8);
    o.write((const char *)gm.data(), gm.size() * sizeof(T));
    o.write((const char *)gv.data(), gv.size() * sizeof(T));
  }
  return 0;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[16];
  f.read((char *)h, sizeof h);
  return h[4] == 0 ? run<float>(f, h, argv[2]) : run<double>(f, h, argv[2]);
}

// Stand-alone driver of the host build of csrc/gmm_em.hip (tests/test_gmm_em_host_cpu.py): gmm_host in.bin out.bin.
// in.bin: int64 N, F, K; double reg_covar; X[N F], weights[K], means[K F], covariances[K F F], resp[N K] (the M-step's input).
// out.bin: U, log_det, resp, log_prob_norm, mean, weights, means, covariances, status, labels -- all as doubles.
#include "gmm_em_host.inc"
#include <fstream>
static std::vector<double> rd(std::ifstream &f, size_t n) { std::vector<double> v(n); f.read((char *)v.data(), n * 8); return v; }
int main(int argc, char **argv) {
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[3]; double reg;
  f.read((char *)h, 24); f.read((char *)&reg, 8);
  const long N = h[0]; const int F = (int)h[1], K = (int)h[2];
  auto X = rd(f, N * F), w = rd(f, K), mu = rd(f, K * F), cov = rd(f, (size_t)K * F * F), rin = rd(f, N * K);
  // exact-size outputs on the heap (ASan)
  std::vector<double> U((size_t)K * F * F, -7.0), ld(K), resp(N * K), lpn(N), mean(1), w2(K), mu2(K * F), cov2((size_t)K * F * F);
  std::vector<int32_t> st(K), lab(N);
  size_t wsb = mlpg_hip_gmm_workspace_bytes(N, F, K);
  std::vector<char> ws(wsb);
  int rc = mlpg_hip_gmm_precisions(0, nullptr, cov.data(), F, K, U.data(), ld.data(), st.data());
  rc |= mlpg_hip_gmm_estep(0, nullptr, X.data(), w.data(), mu.data(), U.data(), ld.data(), N, F, K, resp.data(), lpn.data(), lab.data(), mean.data(), ws.data(), wsb);
  rc |= mlpg_hip_gmm_mstep(0, nullptr, X.data(), rin.data(), N, F, K, reg, w2.data(), mu2.data(), cov2.data(), ws.data(), wsb);
  if (rc) { fprintf(stderr, "rc %d\n", rc); return 1; }
  std::ofstream o(argv[2], std::ios::binary);
  auto wr = [&](const void *p, size_t n) { o.write((const char *)p, n); };
  wr(U.data(), U.size() * 8); wr(ld.data(), K * 8); wr(resp.data(), resp.size() * 8); wr(lpn.data(), N * 8); wr(mean.data(), 8);
  wr(w2.data(), K * 8); wr(mu2.data(), mu2.size() * 8); wr(cov2.data(), cov2.size() * 8);
  std::vector<double> stl(st.begin(), st.end()), labd(lab.begin(), lab.end());
  wr(stl.data(), K * 8); wr(labd.data(), N * 8);
  return 0;
}

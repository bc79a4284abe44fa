// Stand-alone driver of the host builds of csrc/dtw_costs.hip and csrc/dtw.hip (tests/test_dtw_costs_host_cpu.py):
// dtw_costs_host in.bin out.bin.  in.bin: int64 h[8], double eps, then the arrays; every array is an exact-size heap block (ASan).
//   op 0 (launch_dtw_window): h = op, N, radius, path_stride, row_stride; int32 ltx[N], lty[N], full[N], cpath_i[N ps],
//     cpath_j[N ps], cpath_len[N], row_lo[N rs], row_hi[N rs]; int64 row_off[N (rs + 1)].  out: row_lo, row_hi, row_off.
//   op 1 (launch_dtw_costs): h = op, N, tie, path_stride, row_stride, max_ty, total_cells; int32 ltx, lty, row_lo, row_hi; int64
//     row_off; double costs[total_cells]; int64 cost_base[N]; int32 path_i[N ps], path_j[N ps], path_len[N]; double cost[N].
//     out: path_i, path_j, path_len, cost.
//   op 2 (launch_trim): h = op, N, T, D, dtype; X[N T D]; int32 lengths[N].  out: lengths.
//   op 3 (launch_gather): h = op, N, Tsrc, path_stride, D, Tout, dtype; src[N Tsrc D]; int32 path[N ps], path_len[N]; out[N Tout D].
//     out: out.
#include "extras.h"
#include "csrc/x/dtw_costs_host.inc"
#include "csrc/x/dtw_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
template <typename T>
static void wr(std::ofstream &o, const std::vector<T> &v) { o.write((const char *)v.data(), v.size() * sizeof(T)); }
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[8];
  double eps;
  f.read((char *)h, sizeof h);
  f.read((char *)&eps, 8);
  std::ofstream o(argv[2], std::ios::binary);
  const size_t N = (size_t)h[1];
  int rc = 0;
  if (h[0] == 0) {
    const size_t ps = (size_t)h[3], rs = (size_t)h[4];
    auto ltx = rd<int32_t>(f, N), lty = rd<int32_t>(f, N), full = rd<int32_t>(f, N);
    auto ci = rd<int32_t>(f, N * ps), cj = rd<int32_t>(f, N * ps), cl = rd<int32_t>(f, N);
    auto lo = rd<int32_t>(f, N * rs), hi = rd<int32_t>(f, N * rs);
    auto off = rd<int64_t>(f, N * (rs + 1));
    rc = mlpg::launch_dtw_window(nullptr, 0, (int)N, (int)h[2], ltx.data(), lty.data(), full.data(), ci.data(), cj.data(), cl.data(), (int)ps,
                                 lo.data(), hi.data(), off.data(), (int)rs);
    wr(o, lo); wr(o, hi); wr(o, off);
  } else if (h[0] == 1) {
    const size_t ps = (size_t)h[3], rs = (size_t)h[4];
    auto ltx = rd<int32_t>(f, N), lty = rd<int32_t>(f, N);
    auto lo = rd<int32_t>(f, N * rs), hi = rd<int32_t>(f, N * rs);
    auto off = rd<int64_t>(f, N * (rs + 1));
    auto costs = rd<double>(f, (size_t)h[6]);
    auto base = rd<int64_t>(f, N);
    auto pi = rd<int32_t>(f, N * ps), pj = rd<int32_t>(f, N * ps), pl = rd<int32_t>(f, N);
    auto cost = rd<double>(f, N);
    rc = mlpg::launch_dtw_costs(nullptr, 0, (int)N, (int)h[2], ltx.data(), lty.data(), lo.data(), hi.data(), off.data(), (int)rs, (int)h[5],
                                costs.data(), base.data(), h[6], pi.data(), pj.data(), pl.data(), (int)ps, cost.data());
    wr(o, pi); wr(o, pj); wr(o, pl); wr(o, cost);
  } else if (h[0] == 2) {
    const size_t n = N * h[2] * h[3];
    std::vector<int32_t> len;
    if (h[4] == 0) { auto X = rd<float>(f, n); len = rd<int32_t>(f, N); rc = mlpg::launch_trim(nullptr, 0, X.data(), (int)N, (int)h[2], (int)h[3], eps, len.data()); }
    else { auto X = rd<double>(f, n); len = rd<int32_t>(f, N); rc = mlpg::launch_trim(nullptr, 1, X.data(), (int)N, (int)h[2], (int)h[3], eps, len.data()); }
    wr(o, len);
  } else {
    const size_t ps = (size_t)h[3], ns = N * h[2] * h[4], no = N * h[5] * h[4];
    if (h[6] == 0) {
      auto src = rd<float>(f, ns); auto path = rd<int32_t>(f, N * ps), pl = rd<int32_t>(f, N); auto out = rd<float>(f, no);
      rc = mlpg::launch_gather(nullptr, 0, src.data(), path.data(), pl.data(), (int)N, (int)h[2], (int)ps, (int)h[4], (int)h[5], out.data());
      wr(o, out);
    } else {
      auto src = rd<double>(f, ns); auto path = rd<int32_t>(f, N * ps), pl = rd<int32_t>(f, N); auto out = rd<double>(f, no);
      rc = mlpg::launch_gather(nullptr, 1, src.data(), path.data(), pl.data(), (int)N, (int)h[2], (int)ps, (int)h[4], (int)h[5], out.data());
      wr(o, out);
    }
  }
  if (rc) { fprintf(stderr, "launch rc %d\n", rc); return 1; }
  return 0;
}

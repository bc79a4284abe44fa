// Stand-alone driver of the host builds of csrc/mlpg_vargrad.hip and csrc/mlpg_streams_bwd.hip (tests/test_vargrad_host_cpu.py):
// vargrad_host in.bin out.bin.
// in.bin: int64 op, dtype, mode, B, Tmax, sd, ld_in, ld_out, ld_status, members, nw, has_lengths, has_grad_var, has_status,
//   var_elems; int32 members[5][members] (begin, in_col, out_col, sd, stat_col); int32 l[nw], u[nw]; double c[sum(l + u + 1)];
//   int32 lengths[B]; int32 status[B ld_status]; then of dtype: grad_out[B Tmax ld_out] (op 1), var[var_elems],
//   mean[B Tmax ld_in], y[B Tmax ld_out], grad_mean[B Tmax ld_in], grad_var[B Tmax ld_in] (if has_grad_var).
//   op 0 (launch_var_grad): ld_in = nw sd, ld_out = ld_status = sd, no members.  op 1 (launch_streams_bwd): mode 0 / 1 / 3.
// out.bin: grad_mean, grad_var (if has_grad_var), status, as they are after the call.
// Every array is an exact-size heap block (ASan).
#include "extras.h"
#include "csrc/x/mlpg_vargrad_host.inc"
#include "csrc/x/mlpg_streams_bwd_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
template <typename T>
static int run(std::ifstream &f, const int64_t *h, const char *out_path) {
  const int op = (int)h[0], mode = (int)h[2], B = (int)h[3], Tmax = (int)h[4], sd = (int)h[5], nm = (int)h[9], nw = (int)h[10];
  const int64_t ld_in = h[6], ld_out = h[7], ld_status = h[8];
  auto mem = rd<int32_t>(f, 5 * (size_t)nm);
  auto wl = rd<int32_t>(f, nw), wu = rd<int32_t>(f, nw);
  mlpg::WinSet ws;
  memset(&ws, 0, sizeof ws);
  ws.nw = nw;
  int off = 0;
  for (int w = 0; w < nw; ++w) {
    ws.l[w] = wl[w]; ws.u[w] = wu[w]; ws.off[w] = off;
    off += wl[w] + wu[w] + 1;
    if (wl[w] + wu[w] > ws.q) ws.q = wl[w] + wu[w];
    const int m = wl[w] > wu[w] ? wl[w] : wu[w];
    if (m > ws.mw) ws.mw = m;
  }
  if (off > mlpg::kMaxCoef) return 3;
  auto wc = rd<double>(f, off);
  for (int i = 0; i < off; ++i) ws.c[i] = wc[i];
  mlpg::ColTable ct;
  memset(&ct, 0, sizeof ct);
  ct.n = nm;
  for (int m = 0; m < nm; ++m) {
    ct.begin[m] = mem[m]; ct.in_col[m] = mem[nm + m]; ct.out_col[m] = mem[2 * nm + m]; ct.sd[m] = mem[3 * nm + m]; ct.stat_col[m] = mem[4 * nm + m];
    ct.total = ct.begin[m] + ct.sd[m];
  }
  auto len = rd<int32_t>(f, B);
  auto status = rd<int32_t>(f, (size_t)B * ld_status);
  const size_t n_in = (size_t)B * Tmax * ld_in, n_out = (size_t)B * Tmax * ld_out;
  auto gout = rd<T>(f, op == 1 ? n_out : 0);
  auto var = rd<T>(f, (size_t)h[14]);
  auto mean = rd<T>(f, n_in);
  auto y = rd<T>(f, n_out);
  auto gm = rd<T>(f, n_in);
  auto gv = rd<T>(f, h[12] ? n_in : 0);
  const int32_t *lp = h[11] ? len.data() : nullptr;
  int rc;
  if (op == 0)
    rc = mlpg::launch_var_grad(nullptr, (int)h[1], gm.data(), var.data(), mode, mean.data(), y.data(), lp, status.data(), B, Tmax, sd, ws, gv.data());
  else
    rc = mlpg::launch_streams_bwd(nullptr, (int)h[1], mode, gout.data(), var.data(), mean.data(), y.data(), lp, h[13] ? status.data() : nullptr,
                                  B, Tmax, (long)ld_in, (long)ld_out, (int)ld_status, ct, ws, gm.data(), h[12] ? gv.data() : nullptr);
  if (rc) { fprintf(stderr, "launch rc %d\n", rc); return 1; }
  std::ofstream o(out_path, std::ios::binary);
  o.write((const char *)gm.data(), gm.size() * sizeof(T));
  o.write((const char *)gv.data(), gv.size() * sizeof(T));
  o.write((const char *)status.data(), status.size() * 4);
  return 0;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[15];
  f.read((char *)h, sizeof h);
  return h[1] == 0 ? run<float>(f, h, argv[2]) : run<double>(f, h, argv[2]);
}

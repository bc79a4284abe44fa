// Stand-alone driver of the host build of csrc/joint_rows.hip (tests/test_joint_host_cpu.py): joint_host in.bin out.bin.
// in.bin: int64 B, Tmax, Dx, Dy, ld_x, off_x, ld_y, off_y, dtype_x, dtype_y, dtype_out, num_windows, keep, has_len_x, has_len_y, cap,
// ld_out, off_out; float64 eps; int32 win_l[8], win_u[8]; float64 win_coef[136]; int32 len_x[B], len_y[B]; x[B Tmax ld_x] of
// dtype_x (the batch is its columns off_x .. off_x + Dx - 1); y[B Tmax ld_y] of dtype_y.
// out.bin: int64 offsets[B + 1] (prefilled with -7) and out[cap ld_out] of dtype_out (prefilled with -7; the call gets the pointer
// to its column off_out).  Every array is an exact-size heap block (ASan); the workspace has exactly nnmk_joint_workspace_bytes
// bytes of 0xFF.
#include "extras.h"
#include "csrc/x/joint_rows_host.inc"
#include <fstream>
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[18];
  f.read((char *)h, sizeof h);
  const int B = (int)h[0], Tmax = (int)h[1], Dx = (int)h[2], Dy = (int)h[3], dt_x = (int)h[8], dt_y = (int)h[9], dt_o = (int)h[10];
  const int nw = (int)h[11], keep = (int)h[12];
  const int64_t ld_x = h[4], off_x = h[5], ld_y = h[6], off_y = h[7], cap = h[15], ld_out = h[16], off_out = h[17];
  double eps;
  f.read((char *)&eps, 8);
  std::vector<int32_t> wl(8), wu(8), len_x(B), len_y(B);
  std::vector<double> wc(136);
  f.read((char *)wl.data(), 32);
  f.read((char *)wu.data(), 32);
  f.read((char *)wc.data(), 8 * 136);
  f.read((char *)len_x.data(), 4 * (size_t)B);
  f.read((char *)len_y.data(), 4 * (size_t)B);
  const size_t size_of[2] = {4, 8};
  std::vector<char> x(size_of[dt_x] * B * Tmax * ld_x), y(Dy ? size_of[dt_y] * B * Tmax * ld_y : 0), out(size_of[dt_o] * cap * ld_out);
  f.read(x.data(), x.size());
  f.read(y.data(), y.size());
  if (!f) return 3;
  for (size_t i = 0; i < (size_t)(cap * ld_out); ++i)
    if (dt_o == NNMK_JOINT_F64) ((double *)out.data())[i] = -7.0; else ((float *)out.data())[i] = -7.0f;
  std::vector<int64_t> offsets((size_t)B + 1, -7);
  const int64_t wsb = nnmk_joint_workspace_bytes(B, Tmax);
  std::unique_ptr<unsigned char[]> ws(new unsigned char[wsb ? wsb : 1]);
  memset(ws.get(), 0xFF, wsb);
  const void *xp = x.data() + size_of[dt_x] * off_x, *yp = Dy ? y.data() + size_of[dt_y] * off_y : nullptr;
  const int32_t *lx = h[13] ? len_x.data() : nullptr, *ly = h[14] ? len_y.data() : nullptr;
  int rc = nnmk_joint_count(0, nullptr, dt_x, xp, ld_x, lx, Dx, dt_y, yp, ld_y, ly, Dy, B, Tmax, nw, wl.data(), wu.data(), wc.data(), keep, eps,
                            dt_o, ws.get(), wsb, offsets.data());
  if (rc) { fprintf(stderr, "joint_count rc %d\n", rc); return 1; }
  rc = nnmk_joint_write(0, nullptr, dt_x, xp, ld_x, lx, Dx, dt_y, yp, ld_y, ly, Dy, B, Tmax, nw, wl.data(), wu.data(), wc.data(), ws.get(), wsb,
                        dt_o, cap ? out.data() + size_of[dt_o] * off_out : nullptr, ld_out, cap);
  if (rc) { fprintf(stderr, "joint_write rc %d\n", rc); return 1; }
  fprintf(stderr, "launches %lld\n", nnmk_joint_launch_count());
  std::ofstream o(argv[2], std::ios::binary);
  o.write((const char *)offsets.data(), 8 * offsets.size());
  o.write(out.data(), out.size());
  return 0;
}

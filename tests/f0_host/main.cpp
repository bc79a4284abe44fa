// Stand-alone driver of the host build of csrc/f0_interp.hip (tests/test_f0_host_cpu.py): f0_host in.bin out.bin.
// in.bin: int64 B, Tmax, C, ld_x, off_x, ld_y, off_y, ld_v, off_v, dtype_x, dtype_y, dtype_vuv, kind, has_lengths, mode;
// int32 lengths[B]; x[B Tmax ld_x] of dtype_x (the batch is its columns off_x .. off_x + C - 1).
// mode: 0 y and vuv, 1 y only, 2 vuv only, 3 in place (y is x) with vuv, 4 in place without.
// out.bin: x[B Tmax ld_x] as it is after the call, y[B Tmax ld_y] of dtype_y and vuv[B Tmax ld_v] of dtype_vuv (both prefilled
// with -7; the call gets the pointers to their columns off_y / off_v).  Every array is an exact-size heap block (ASan).
#include "extras.h"
#include "csrc/x/f0_interp_host.inc"
#include <fstream>
static void fill(std::vector<char> &v, int dt, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (dt == NNMK_F0_F64) ((double *)v.data())[i] = -7.0; else ((float *)v.data())[i] = -7.0f;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[15];
  f.read((char *)h, sizeof h);
  const int B = (int)h[0], Tmax = (int)h[1], C = (int)h[2], dt_x = (int)h[9], dt_y = (int)h[10], dt_v = (int)h[11], kind = (int)h[12];
  const int mode = (int)h[14];
  const int64_t ld_x = h[3], off_x = h[4], ld_y = h[5], off_y = h[6], ld_v = h[7], off_v = h[8];
  const size_t size_of[2] = {4, 8};
  std::vector<char> lengths(4 * (size_t)B);
  f.read(lengths.data(), lengths.size());
  const size_t n_x = (size_t)B * Tmax * ld_x, n_y = (size_t)B * Tmax * ld_y, n_v = (size_t)B * Tmax * ld_v;
  std::vector<char> x(size_of[dt_x] * n_x), y(size_of[dt_y] * n_y), v(size_of[dt_v] * n_v);
  f.read(x.data(), x.size());
  fill(y, dt_y, n_y);
  fill(v, dt_v, n_v);
  const bool in_place = mode == 3 || mode == 4;
  void *yp = mode == 2 ? nullptr : (in_place ? x.data() + size_of[dt_x] * off_x : y.data() + size_of[dt_y] * off_y);
  void *vp = mode == 1 || mode == 4 ? nullptr : v.data() + size_of[dt_v] * off_v;
  const int rc = nnmk_f0_interp(0, nullptr, dt_x, x.data() + size_of[dt_x] * off_x, ld_x, h[13] ? (const int32_t *)lengths.data() : nullptr, B,
                                Tmax, C, kind, in_place ? dt_x : dt_y, yp, in_place ? ld_x : ld_y, dt_v, vp, ld_v);
  if (rc) { fprintf(stderr, "f0_interp rc %d\n", rc); return 1; }
  fprintf(stderr, "launches %lld\n", nnmk_f0_launch_count());
  std::ofstream o(argv[2], std::ios::binary);
  o.write(x.data(), x.size());
  o.write(y.data(), y.size());
  o.write(v.data(), v.size());
  return 0;
}

// Stand-alone driver of the host build of csrc/wave_codec.hip (tests/test_wave_host_cpu.py): wave_host in.bin out.bin.
// in.bin: int64 op (0 encode, 1 decode), B, Lmax, ld_x, off_x, ld_y, off_y, dtype_x, dtype_y, has_lengths, in_place, emphasis,
// stage, mu, segment, n_table; double coef; int32 lengths[B]; float table[n_table]; x[B ld_x] of dtype_x; y[B ld_y] of dtype_y
// as it is before the call (the batch is at elements off .. off + Lmax - 1 of each row).  in_place: y is x.
// out.bin: int64 rc, launches; x and y as they are after the call.  Every array is an exact-size heap block (ASan).
#include "extras.h"
#include "csrc/x/wave_codec_host.inc"
#include <fstream>
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[16];
  double coef;
  f.read((char *)h, sizeof h);
  f.read((char *)&coef, sizeof coef);
  const int op = (int)h[0], B = (int)h[1], Lmax = (int)h[2], dt_x = (int)h[7], dt_y = (int)h[8], emphasis = (int)h[11], stage = (int)h[12];
  const int mu = (int)h[13];
  const int64_t ld_x = h[3], off_x = h[4], ld_y = h[5], off_y = h[6], segment = h[14], n_table = h[15];
  const size_t size_of[6] = {4, 8, 1, 2, 4, 8};
  std::vector<char> lengths(4 * (size_t)B), table(4 * (size_t)n_table), x(size_of[dt_x] * B * ld_x), y(size_of[dt_y] * B * ld_y);
  f.read(lengths.data(), lengths.size());
  f.read(table.data(), table.size());
  f.read(x.data(), x.size());
  f.read(y.data(), y.size());
  if (!f) return 3;
  void *xp = x.data() + size_of[dt_x] * off_x;
  void *yp = h[10] ? xp : (void *)(y.data() + size_of[dt_y] * off_y);
  const int32_t *lp = h[9] ? (const int32_t *)lengths.data() : nullptr;
  int64_t rc;
  if (op == 0)
    rc = nnmk_wave_encode(0, nullptr, dt_x, xp, ld_x, lp, B, Lmax, emphasis, coef, stage, mu, dt_y, yp, h[10] ? ld_x : ld_y);
  else
    rc = nnmk_wave_decode(0, nullptr, dt_x, xp, ld_x, lp, B, Lmax, stage, mu, n_table ? (const float *)table.data() : nullptr, emphasis, coef,
                          segment, dt_y, yp, h[10] ? ld_x : ld_y);
  const int64_t launches = nnmk_wave_launch_count();
  std::ofstream o(argv[2], std::ios::binary);
  o.write((const char *)&rc, sizeof rc);
  o.write((const char *)&launches, sizeof launches);
  o.write(x.data(), x.size());
  o.write(y.data(), y.size());
  return 0;
}

// Stand-alone driver of the host build of csrc/frame_expand.hip (tests/test_frontend_host_cpu.py): frontend_host in.bin out.bin.
// in.bin: int64 B, Nmax, S, Dl, ld_p, dtype_phone, dtype_dur, has_num_phones, min_frames, kind, affine, dtype_out, ld_out, Tmax;
// int32 num_phones[B]; phone[B Nmax ld_p] of dtype_phone; durations[B Nmax S] of dtype_dur; double cc[3 600] for kind 6;
// double scale[Dl + F], min[Dl + F] if affine.
// out.bin: out[B Tmax ld_out] of dtype_out (prefilled with -7), int32 lengths[B], int64 counts[B] (both prefilled with -7).
// Every array is an exact-size heap block (ASan).
#include "extras.h"
#include "csrc/x/frame_expand_host.inc"
#include <fstream>
static std::vector<char> rd(std::ifstream &f, size_t bytes) { std::vector<char> v(bytes); f.read(v.data(), bytes); return v; }
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[14];
  f.read((char *)h, sizeof h);
  const int B = (int)h[0], Nmax = (int)h[1], S = (int)h[2], Dl = (int)h[3], dt_p = (int)h[5], dt_d = (int)h[6], kind = (int)h[9];
  const int dt_o = (int)h[11], Tmax = (int)h[13];
  const int64_t ld_p = h[4], ld_out = h[12];
  const size_t size_of[4] = {4, 8, 4, 8};
  const int F = nnmk_frontend_feature_size(kind);
  if (F < 0) return 3;
  auto np = rd(f, 4 * (size_t)B);
  auto phone = rd(f, size_of[dt_p] * B * Nmax * ld_p);
  auto dur = rd(f, size_of[dt_d] * B * Nmax * S);
  auto cc = rd(f, kind == NNMK_FRONTEND_COARSE_CODING ? 8 * 3 * NNMK_FRONTEND_CC_POINTS : 0);
  auto scale = rd(f, h[10] ? 8 * (size_t)(Dl + F) : 0), mins = rd(f, h[10] ? 8 * (size_t)(Dl + F) : 0);
  const size_t n_out = (size_t)B * Tmax * ld_out;
  std::vector<char> out(size_of[dt_o] * n_out);
  for (size_t i = 0; i < n_out; ++i)
    if (dt_o == NNMK_FRONTEND_F64) ((double *)out.data())[i] = -7.0; else ((float *)out.data())[i] = -7.0f;
  std::vector<int32_t> lengths(B, -7);
  std::vector<int64_t> counts(B, -7);
  const int32_t *npp = h[7] ? (const int32_t *)np.data() : nullptr;
  int rc = nnmk_frontend_frame_counts(0, nullptr, dt_d, dur.data(), npp, B, Nmax, S, (int)h[8], counts.data());
  if (rc) { fprintf(stderr, "frame_counts rc %d\n", rc); return 1; }
  rc = nnmk_frontend_expand(0, nullptr, dt_p, phone.data(), ld_p, dt_d, dur.data(), npp, B, Nmax, S, Dl, (int)h[8], kind,
                            cc.empty() ? nullptr : (const double *)cc.data(), h[10] ? (const double *)scale.data() : nullptr,
                            h[10] ? (const double *)mins.data() : nullptr, dt_o, out.data(), ld_out, Tmax, lengths.data());
  if (rc) { fprintf(stderr, "expand rc %d\n", rc); return 1; }
  std::ofstream o(argv[2], std::ios::binary);
  o.write(out.data(), out.size());
  o.write((const char *)lengths.data(), 4 * (size_t)B);
  o.write((const char *)counts.data(), 8 * (size_t)B);
  return 0;
}

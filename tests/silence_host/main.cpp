// Stand-alone driver of the host build of csrc/frame_keep.hip (tests/test_silence_host_cpu.py): silence_host in.bin out.bin.
// in.bin: int64 B, Nmax, S, Dl, ld_p, dtype_phone, dtype_dur, has_num_phones, min_frames, kind, affine, dtype_out, ld_out, Tcap,
// do_gather, Tmax, D, ld_src, dtype_src, has_len_src, ld_gout, Tcap_gather; int32 num_phones[B]; uint8 silence[B Nmax];
// phone[B Nmax ld_p] of dtype_phone; durations[B Nmax S] of dtype_dur; double cc[3 600] for kind 6; double scale[Dl + F],
// min[Dl + F] if affine; if do_gather: int32 len_src[B], src[B Tmax ld_src] of dtype_src.
// out.bin: out[B Tcap ld_out] of dtype_out (prefilled with -7), int32 lengths[B], int64 counts[B 2] (both prefilled with -7); if
// do_gather: gout[B Tcap_gather ld_gout] of dtype_out (prefilled with -7), int32 glengths[B] (-7).
// Every array is an exact-size heap block (ASan).
#include "extras.h"
#include "csrc/x/frame_keep_host.inc"
#include <fstream>
static std::vector<char> rd(std::ifstream &f, size_t bytes) { std::vector<char> v(bytes); f.read(v.data(), bytes); return v; }
static std::vector<char> filled(int dt, size_t n) {
  std::vector<char> v((dt == NNMK_FRONTEND_F64 ? 8 : 4) * n);
  for (size_t i = 0; i < n; ++i)
    if (dt == NNMK_FRONTEND_F64) ((double *)v.data())[i] = -7.0; else ((float *)v.data())[i] = -7.0f;
  return v;
}
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[22];
  f.read((char *)h, sizeof h);
  const int B = (int)h[0], Nmax = (int)h[1], S = (int)h[2], Dl = (int)h[3], dt_p = (int)h[5], dt_d = (int)h[6], kind = (int)h[9];
  const int dt_o = (int)h[11], Tcap = (int)h[13], Tmax = (int)h[15], D = (int)h[16], dt_s = (int)h[18], Tcap_g = (int)h[21];
  const int64_t ld_p = h[4], ld_out = h[12], ld_src = h[17], ld_gout = h[20];
  const size_t size_of[4] = {4, 8, 4, 8};
  const int F = sk_feature_size(kind);   // (the text's own table)
  if (F < 0) return 3;
  auto np = rd(f, 4 * (size_t)B);
  auto sil = rd(f, (size_t)B * Nmax);
  auto phone = rd(f, size_of[dt_p] * B * Nmax * ld_p);
  auto dur = rd(f, size_of[dt_d] * B * Nmax * S);
  auto cc = rd(f, kind == NNMK_FRONTEND_COARSE_CODING ? 8 * 3 * NNMK_FRONTEND_CC_POINTS : 0);
  auto scale = rd(f, h[10] ? 8 * (size_t)(Dl + F) : 0), mins = rd(f, h[10] ? 8 * (size_t)(Dl + F) : 0);
  auto len = rd(f, h[14] ? 4 * (size_t)B : 0);
  auto src = rd(f, h[14] ? size_of[dt_s] * B * Tmax * ld_src : 0);
  auto out = filled(dt_o, (size_t)B * Tcap * ld_out);
  std::vector<int32_t> lengths(B, -7), glengths(B, -7);
  std::vector<int64_t> counts(2 * (size_t)B, -7);
  const int32_t *npp = h[7] ? (const int32_t *)np.data() : nullptr;
  const uint8_t *silp = (const uint8_t *)sil.data();
  int rc = nnmk_sil_frame_counts(0, nullptr, dt_d, dur.data(), npp, silp, B, Nmax, S, (int)h[8], counts.data());
  if (rc) { fprintf(stderr, "frame_counts rc %d\n", rc); return 1; }
  rc = nnmk_sil_expand(0, nullptr, dt_p, phone.data(), ld_p, dt_d, dur.data(), npp, silp, B, Nmax, S, Dl, (int)h[8], kind,
                       cc.empty() ? nullptr : (const double *)cc.data(), h[10] ? (const double *)scale.data() : nullptr,
                       h[10] ? (const double *)mins.data() : nullptr, dt_o, out.data(), ld_out, Tcap, lengths.data());
  if (rc) { fprintf(stderr, "expand rc %d\n", rc); return 1; }
  std::ofstream o(argv[2], std::ios::binary);
  o.write(out.data(), out.size());
  o.write((const char *)lengths.data(), 4 * (size_t)B);
  o.write((const char *)counts.data(), 16 * (size_t)B);
  if (h[14]) {
    auto gout = filled(dt_o, (size_t)B * Tcap_g * ld_gout);
    rc = nnmk_sil_gather(0, nullptr, dt_d, dur.data(), npp, silp, B, Nmax, S, (int)h[8], dt_s, src.data(), ld_src,
                         h[19] ? (const int32_t *)len.data() : nullptr, Tmax, D, dt_o, gout.data(), ld_gout, Tcap_g, glengths.data());
    if (rc) { fprintf(stderr, "gather rc %d\n", rc); return 1; }
    o.write(gout.data(), gout.size());
    o.write((const char *)glengths.data(), 4 * (size_t)B);
  }
  return 0;
}

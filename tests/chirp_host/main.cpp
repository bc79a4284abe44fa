// Stand-alone driver of the host build of csrc/modspec_chirp.hip (tests/test_modspec_chirp_host_cpu.py): chirp_host in.bin out.bin.
// in.bin: int64 mode, B, T, D, n, ortho, limit_bin, log_domain, want_phase; then double arrays, nb = n/2 + 1:
//   mode 0 (spectrum) x[B T D]; 1 (inverse) ms[B nb D], ph[B nb D 2]; 2 (smoothing) x[B T D]; 3 (backward) x[B T D], g[B nb D].
// out.bin: out (0: [B nb D]; 1: [B n D]; 2, 3: [B T D]), then for mode 0 with want_phase out_ph[B nb D 2]; prefilled with -7.
// Every array is an exact-size heap block (ASan); so are the dynamic LDS of every launch and the scratch with the two tables.
#include "extras.h"
#include "csrc/x/modspec_chirp_host.inc"
#include <fstream>
static std::vector<double> rd(std::ifstream &f, size_t n) { std::vector<double> v(n); f.read((char *)v.data(), n * 8); return v; }
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[9];
  f.read((char *)h, sizeof h);
  const int mode = (int)h[0], B = (int)h[1], T = (int)h[2], D = (int)h[3], n = (int)h[4];
  const size_t nb = (size_t)n / 2 + 1, BD = (size_t)B * D;
  auto x = rd(f, mode == 1 ? 0 : BD * T);
  auto ms = rd(f, mode == 1 || mode == 3 ? BD * nb : 0);
  auto ph = rd(f, mode == 1 ? BD * nb * 2 : 0);
  std::vector<double> out(BD * (mode == 0 ? nb : mode == 1 ? (size_t)n : (size_t)T), -7.0);
  std::vector<double> out_ph(mode == 0 && h[8] ? BD * nb * 2 : 0, -7.0);
  const int rc = mlpg::launch_modspec_chirp(nullptr, 0, mode, x.empty() ? nullptr : x.data(), ms.empty() ? nullptr : ms.data(),
                                            ph.empty() ? nullptr : ph.data(), out.data(), out_ph.empty() ? nullptr : out_ph.data(), B, T,
                                            D, n, (int)h[5], (int)h[6], (int)h[7]);
  if (rc) { fprintf(stderr, "launch_modspec_chirp rc %d\n", rc); return 1; }
  std::ofstream o(argv[2], std::ios::binary);
  o.write((const char *)out.data(), out.size() * 8);
  o.write((const char *)out_ph.data(), out_ph.size() * 8);
  return 0;
}

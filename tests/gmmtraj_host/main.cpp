// Stand-alone driver of the host build of csrc/gmm_traj.hip (tests/test_gmmtraj_host_cpu.py): gmmtraj_host in.bin out.bin.
// in.bin: int64 B, Tmax, D, M, ld_x, ld_out, has_lengths; int32 lengths[B], labels[B Tmax]; double x[B Tmax ld_x], mu_x[M D],
// mu_y[M D], A[M D D], cvar[M D].  out.bin: mean[B Tmax ld_out], var[B Tmax ld_out] (prefilled with -7: untouched columns keep it).
#include "extras.h"
#include "gmm_traj_host.inc"
#include <fstream>
template <typename T>
static std::vector<T> rd(std::ifstream &f, size_t n) { std::vector<T> v(n); f.read((char *)v.data(), n * sizeof(T)); return v; }
int main(int argc, char **argv) {
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[7];
  f.read((char *)h, sizeof h);
  const int B = (int)h[0], T = (int)h[1], D = (int)h[2], M = (int)h[3];
  const int64_t ldx = h[4], ldo = h[5];
  const size_t rows = (size_t)B * T;
  auto len = rd<int32_t>(f, B), lab = rd<int32_t>(f, rows);
  // exact-size arrays on the heap (ASan): the last row of x and of the outputs ends at its D-th column
  auto x = rd<double>(f, rows * ldx);
  x.resize(rows ? (rows - 1) * ldx + D : 0);
  x.shrink_to_fit();
  auto mux = rd<double>(f, (size_t)M * D), muy = rd<double>(f, (size_t)M * D), A = rd<double>(f, (size_t)M * D * D), cv = rd<double>(f, (size_t)M * D);
  std::vector<double> mean(rows ? (rows - 1) * ldo + D : 0, -7.0), var(mean.size(), -7.0);
  int rc = mlpg_hip_gmm_trajectory_stats(0, nullptr, x.data(), ldx, h[6] ? len.data() : nullptr, B, T, D, lab.data(), mux.data(), muy.data(),
                                         A.data(), cv.data(), M, mean.data(), ldo, var.data(), ldo);
  if (rc) { fprintf(stderr, "rc %d\n", rc); return 1; }
  mean.resize(rows * ldo, -7.0);
  var.resize(rows * ldo, -7.0);
  std::ofstream o(argv[2], std::ios::binary);
  o.write((const char *)mean.data(), mean.size() * 8);
  o.write((const char *)var.data(), var.size() * 8);
  return 0;
}

// Stand-alone driver of the host build of csrc/kmeans.hip (tests/test_kmeans_host_cpu.py): kmeans_host in.bin out.bin.
// in.bin: int64 N, F, K, C; X[N F], shift[F], closest[N], centers[K F] as doubles; candidates[C], labels_prev[N] as int64.
// out.bin, all as doubles: the seed step without closest_in (d[C N], pots[C]) and with it (d[C N], pots[C]); the Lloyd step with
// the centre update (labels[N], min_dist[N], sums[K F], counts[K], centers_out[K F], shift, inertia, changed, empty); the step
// without it, started from the labels just found (labels[N], shift, inertia, changed, empty).
#include "common.h"
namespace mlpg { enum { kCountKmeansSeed = 26, kCountKmeansLloyd }; }
#include "kmeans_host.inc"
#include <fstream>
static std::vector<double> rd(std::ifstream &f, size_t n) { std::vector<double> v(n); f.read((char *)v.data(), n * 8); return v; }
static std::vector<int32_t> rdi(std::ifstream &f, size_t n) { std::vector<int64_t> v(n); f.read((char *)v.data(), n * 8); return std::vector<int32_t>(v.begin(), v.end()); }
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int64_t h[4];
  f.read((char *)h, 32);
  const long N = h[0]; const int F = (int)h[1], K = (int)h[2], C = (int)h[3];
  auto X = rd(f, N * F), shift = rd(f, F), closest = rd(f, N), cen = rd(f, K * F);
  auto cand = rdi(f, C), prev = rdi(f, N);
  // exact-size arrays on the heap (ASan)
  std::vector<double> d0((size_t)C * N), p0(C), d1((size_t)C * N), p1(C), md(N), sums(K * F), counts(K), cout_(K * F), sums2(K * F), counts2(K);
  std::vector<int32_t> lab(N), lab2(N);
  struct Stats { double shift, inertia; long long changed, empty; } st1, st2;
  const size_t wsb = mlpg_hip_kmeans_workspace_bytes(N, F, K);
  std::vector<char> ws(wsb);
  int rc = mlpg_hip_kmeans_seed_step(0, nullptr, X.data(), shift.data(), N, F, cand.data(), C, nullptr, d0.data(), p0.data(), ws.data(), wsb);
  rc |= mlpg_hip_kmeans_seed_step(0, nullptr, X.data(), shift.data(), N, F, cand.data(), C, closest.data(), d1.data(), p1.data(), ws.data(), wsb);
  rc |= mlpg_hip_kmeans_lloyd_step(0, nullptr, X.data(), shift.data(), cen.data(), prev.data(), N, F, K, 1, lab.data(), md.data(), sums.data(), counts.data(), cout_.data(), &st1, ws.data(), wsb);
  rc |= mlpg_hip_kmeans_lloyd_step(0, nullptr, X.data(), shift.data(), cen.data(), lab.data(), N, F, K, 0, lab2.data(), nullptr, sums2.data(), counts2.data(), nullptr, &st2, ws.data(), wsb);
  if (rc) { fprintf(stderr, "rc %d\n", rc); return 1; }
  std::ofstream o(argv[2], std::ios::binary);
  auto wr = [&](const std::vector<double> &v) { o.write((const char *)v.data(), v.size() * 8); };
  wr(d0); wr(p0); wr(d1); wr(p1);
  wr(std::vector<double>(lab.begin(), lab.end())); wr(md); wr(sums); wr(counts); wr(cout_);
  wr({st1.shift, st1.inertia, (double)st1.changed, (double)st1.empty});
  wr(std::vector<double>(lab2.begin(), lab2.end()));
  wr({st2.shift, st2.inertia, (double)st2.changed, (double)st2.empty});
  return 0;
}

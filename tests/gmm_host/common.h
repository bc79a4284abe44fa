// Host stand-in for csrc/common.h and the HIP runtime (tests/test_gmm_em_host_cpu.py): the unchanged text of csrc/gmm_em.hip is
// compiled for the CPU against it.  A workgroup is a set of std::threads on a barrier, a wave 64 of them; the wave-wide operations
// (the xor shuffle and v_mfma_f64_16x16x4_f64, with the lane maps of DESIGN.md K6) exchange their operands through per-wave
// arrays; dynamic LDS is an exact-size heap block, so the address sanitizer sees an access past it.
#pragma once
#include <barrier>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
#define MLPG_HIP_EINVAL (-1)
#define MLPG_HIP_ERUNTIME (-2)
typedef void *hipStream_t;
typedef int hipError_t;
constexpr int hipSuccess = 0;
constexpr int hipFuncAttributeMaxDynamicSharedMemorySize = 0;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct Idx { unsigned x, y, z; };
inline thread_local Idx threadIdx, blockIdx;
inline double *g_dyn_lds = nullptr;
inline std::barrier<> *g_block_bar = nullptr;
inline std::vector<std::unique_ptr<std::barrier<>>> g_wave_bar;
inline double g_xa[8][64], g_xb[8][64];
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
inline double __shfl_xor(double v, int m) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_xa[w][l] = v;
  g_wave_bar[w]->arrive_and_wait();
  const double r = g_xa[w][l ^ m];
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
typedef double v4d_shim __attribute__((ext_vector_type(4)));
// v_mfma_f64_16x16x4_f64: lane l gives A[l & 15][l >> 4], B[l >> 4][l & 15]; register g of lane l is D[(l >> 4) + 4 g][l & 15]
inline v4d_shim __builtin_amdgcn_mfma_f64_16x16x4f64(double a, double b, v4d_shim c, int, int, int) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_xa[w][l] = a;
  g_xb[w][l] = b;
  g_wave_bar[w]->arrive_and_wait();
  for (int g = 0; g < 4; ++g) {
    const int row = (l >> 4) + 4 * g, col = l & 15;
    double s = c[g];
    for (int k = 0; k < 4; ++k) s += g_xa[w][k * 16 + row] * g_xb[w][k * 16 + col];
    c[g] = s;
  }
  g_wave_bar[w]->arrive_and_wait();
  return c;
}
inline int min(int a, int b) { return a < b ? a : b; }
inline int hipFuncSetAttribute(const void *, int, int) { return 0; }
inline int hipGetLastError() { return 0; }
inline const char *hipGetErrorString(int) { return ""; }
template <typename K, typename... A>
void hipLaunchKernelGGL(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t, A... args) {
  // exact-size dynamic LDS so that the address sanitizer sees an access past it; the workgroups run one after another on one set
  // of threads, with a barrier between them (static __shared__ arrays are reused)
  std::unique_ptr<double[]> exact(new double[lds / 8 + (lds ? 0 : 1)]);
  g_dyn_lds = exact.get();
  std::barrier<> bb(block.x);
  g_block_bar = &bb;
  g_wave_bar.clear();
  for (unsigned w = 0; w < (block.x + 63) / 64; ++w)
    g_wave_bar.emplace_back(new std::barrier<>(64 < block.x - 64 * w ? 64 : block.x - 64 * w));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < block.x; ++t)
    th.emplace_back([=] {
      for (unsigned bz = 0; bz < grid.z; ++bz)
        for (unsigned by = 0; by < grid.y; ++by)
          for (unsigned bx = 0; bx < grid.x; ++bx) {
            threadIdx = Idx{t, 0, 0};
            blockIdx = Idx{bx, by, bz};
            kern(args...);
            g_block_bar->arrive_and_wait();
          }
    });
  for (auto &t : th) t.join();
}
namespace mlpg {
constexpr int kMaxDevices = 16;
enum { kCountGmmEstep = 22, kCountGmmMstep, kCountGmmPrecisions };
inline void note_launch(int) {}
inline void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
inline int check_device(const char *, int d) { return d >= 0 && d < kMaxDevices ? 0 : -1; }
struct DeviceGuard { int rc = 0; DeviceGuard(const char *, int) {} };
}
#define MLPG_HIP_CHECK(expr) do { if ((expr) != 0) return -2; } while (0)

// Host stand-in for csrc/common.h and the HIP runtime (tests/test_*_host_cpu.py, first tests/test_gmm_em_host_cpu.py): the
// unchanged text of a .hip file is compiled for the CPU against it.  A workgroup is a set of std::threads on a barrier, a wave 64
// of them; the wave-wide operations (the shuffles, typed: 8 bytes bit for bit; v_mfma_f64_16x16x4_f64, with the lane maps of
// DESIGN.md K6) exchange their operands through per-wave arrays; dynamic LDS is a heap block of exactly the requested bytes and
// mlpg::scratch() a fresh exact-size block of 0xFF bytes, so the address sanitizer sees an access past either.  What one kernel
// text needs beyond this lives in its program's extras.h.
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
#define __forceinline__ inline
#define __align__(n) alignas(n)
#define MLPG_HIP_EINVAL (-1)
#define MLPG_HIP_ERUNTIME (-2)
typedef void *hipStream_t;
typedef int hipError_t;
constexpr int hipSuccess = 0;
constexpr int hipFuncAttributeMaxDynamicSharedMemorySize = 0;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct Idx { unsigned x, y, z; };
inline thread_local Idx threadIdx, blockIdx;
inline Idx blockDim{1, 1, 1}, gridDim{1, 1, 1};
inline double *g_dyn_lds = nullptr;
inline std::barrier<> *g_block_bar = nullptr;
inline std::vector<std::unique_ptr<std::barrier<>>> g_wave_bar;
inline double g_xa[16][64], g_xb[16][64];   // (a workgroup of 1024 threads is 16 waves)
inline unsigned long long g_xs[16][64];
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
// Shuffles carry their operand bit for bit (8 bytes through the wave's array, no trip through double: a long long sum above 2^53
// survives).  Every lane of the wave calls them; a lane whose source is outside the wave keeps its own value, as on the device.
template <typename T>
inline T shim_lane_read(T v, int src_of(int, int), int arg) {
  static_assert(sizeof(T) <= 8, "shuffles move at most 8 bytes");
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  unsigned long long bits = 0;
  memcpy(&bits, &v, sizeof(T));
  g_xs[w][l] = bits;
  g_wave_bar[w]->arrive_and_wait();
  const int src = src_of(l, arg);
  bits = (src >= 0 && src < 64) ? g_xs[w][src] : bits;
  g_wave_bar[w]->arrive_and_wait();
  T r;
  memcpy(&r, &bits, sizeof(T));
  return r;
}
template <typename T> inline T __shfl_xor(T v, int m) { return shim_lane_read(v, +[](int l, int a) { return l ^ a; }, m); }
template <typename T> inline T __shfl_up(T v, int d) { return shim_lane_read(v, +[](int l, int a) { return l - a; }, d); }
template <typename T> inline T __shfl_down(T v, int d) { return shim_lane_read(v, +[](int l, int a) { return l + a; }, d); }
template <typename T> inline T __shfl(T v, int src) { return shim_lane_read(v, +[](int, int a) { return a; }, src); }
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
struct alignas(16) double2 { double x, y; };
inline double2 make_double2(double x, double y) { return double2{x, y}; }
inline int hipFuncSetAttribute(const void *, int, int) { return 0; }
inline int hipGetLastError() { return 0; }
inline const char *hipGetErrorString(int) { return ""; }
template <typename K, typename... A>
void hipLaunchKernelGGL(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t, A... args) {
  // exact-size dynamic LDS so that the address sanitizer sees an access past it; the workgroups run one after another on one set
  // of threads, with a barrier between them (static __shared__ arrays are reused)
  // (a block of bytes, not of doubles: a size that is no multiple of 8 is exact too; operator new aligns it to 16)
  std::unique_ptr<char[]> exact(new char[lds ? lds : 1]);
  g_dyn_lds = (double *)exact.get();
  blockDim = Idx{block.x, 1, 1};
  gridDim = Idx{grid.x, grid.y, grid.z};
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
// Stand-in for the grow-only scratch of csrc/common.h: every call returns a fresh exact-size heap block (kept until the program
// ends) filled with 0xFF bytes -- NaN as double, -1 as int32 -- so that a read of workspace the call did not write first shows in
// the result, and an access past the requested bytes trips the address sanitizer.
inline std::vector<std::unique_ptr<unsigned char[]>> g_scratch_blocks;
inline void *scratch(int, hipStream_t, int, size_t bytes, unsigned long long *gen = nullptr) {
  g_scratch_blocks.emplace_back(new unsigned char[bytes ? bytes : 1]);
  memset(g_scratch_blocks.back().get(), 0xFF, bytes);
  if (gen) *gen = g_scratch_blocks.size();
  return g_scratch_blocks.back().get();
}
inline void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
inline int check_device(const char *, int d) { return d >= 0 && d < kMaxDevices ? 0 : -1; }
struct DeviceGuard { int rc = 0; DeviceGuard(const char *, int) {} };
}
#define MLPG_HIP_CHECK(expr) do { if ((expr) != 0) return -2; } while (0)

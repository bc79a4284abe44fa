// The in-LDS complex FFT the modulation-spectrum kernels share (modspec.hip: power-of-two DFT lengths; modspec_chirp.hip: the
// chirp-z transform of every other length up to 2048 and the kernel that builds its filter spectrum): the padded LDS layout, the
// per-pass twiddle tables, the radix-16 / radix-8 first pass in registers and the radix-4 passes, the bit reversal, the packing
// of two real columns into one complex sequence, and the four modes of the float64 entries.  Device code only, one copy per
// translation unit.
//
// FFT: in-place decimation in time on bit-reversed input.  First pass: a radix-16 (radix-8 for odd
// log2 n) transform of 16 consecutive elements in registers; then radix-4 passes (two radix-2
// stages fused).  The data are padded by one slot per 16 elements and every pass has its own compact
// twiddle table (sincospi, float64), so that no LDS access of the transform has a bank conflict
// by construction.
#pragma once
#include <math.h>

#include "common.h"

namespace mlpg {
namespace {

struct Cplx {
  double re, im;
};
__device__ __forceinline__ Cplx cadd(Cplx a, Cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ Cplx csub(Cplx a, Cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ Cplx cmul(Cplx a, Cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

constexpr int kFftThreads = 1024;

// LDS layout: element i lives at a[pidx(i)], one padding slot per 16 elements, so that both the
// first pass (every thread owns 8 or 16 CONSECUTIVE elements) and the later passes (consecutive
// threads touch consecutive elements) are free of bank conflicts.
__device__ __forceinline__ int pidx(int i) { return i + (i >> 4); }
constexpr int padded_len(int n) { return n + (n >> 4) + 1; }

// Twiddles: one compact table per radix-4 pass (stages s, s+1; h = 2^s): tab[j] = W_{4h}^j, j < 2h,
// read by consecutive threads at consecutive addresses.  Pass tables are stored back to back;
// tw_offset(s0, s) = 2 * (h(s0) + h(s0 + 2) + ... below s) entries.
__device__ __forceinline__ int tw_offset(int s0, int s) {
  int off = 0;
  for (int t = s0; t < s; t += 2) off += 2 << t;
  return off;
}

// In-register DIT FFT of R = 2^LOGR consecutive elements (input in bit-reversed order), W_R = exp(-+ 2 pi i / R)
template <int LOGR, bool INV>
__device__ __forceinline__ void fft_regs(Cplx (&v)[1 << LOGR]) {
  constexpr int R = 1 << LOGR;
  // cos / sin of 2 pi k / 16, k = 0..7
  constexpr double c16[8] = {1.0, 0.92387953251128673848, 0.70710678118654752440, 0.38268343236508977173,
                             0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128673848};
  constexpr double s16[8] = {0.0, 0.38268343236508977173, 0.70710678118654752440, 0.92387953251128673848,
                             1.0, 0.92387953251128673848, 0.70710678118654752440, 0.38268343236508977173};
#pragma unroll
  for (int t = 0; t < LOGR; ++t) {
    const int h = 1 << t;
#pragma unroll
    for (int b = 0; b < R / 2; ++b) {
      const int j = b & (h - 1);
      const int i0 = ((b >> t) << (t + 1)) | j;
      const int k16 = j * (8 >> t);  // W_{2h}^j = W_16^{j * 16 / (2h)}
      const Cplx w = {c16[k16], INV ? s16[k16] : -s16[k16]};
      const Cplx u = v[i0], x = (k16 == 0) ? v[i0 + h] : cmul(v[i0 + h], w);
      v[i0] = cadd(u, x);
      v[i0 + h] = csub(u, x);
    }
  }
}

// The radix-16 first pass for the kernels of the padded-minibatch entries, in two sweeps over the thread's own 16 consecutive
// elements (no barrier between them): stages 0-1 on four groups of four, stages 2-3 on the elements j, j+4, j+8, j+12.  The same
// butterflies as fft_regs<4>, with 4 instead of 16 complex values live at a time: next to the typed loads and stores and the loss
// arithmetic, 16 live values push those kernels past the 128 registers a 1024-thread workgroup leaves a lane.
template <bool INV>
__device__ __forceinline__ void fft16_two_sweeps(Cplx *a, int q) {
  constexpr double c16[8] = {1.0, 0.92387953251128673848, 0.70710678118654752440, 0.38268343236508977173,
                             0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128673848};
  constexpr double s16[8] = {0.0, 0.38268343236508977173, 0.70710678118654752440, 0.92387953251128673848,
                             1.0, 0.92387953251128673848, 0.70710678118654752440, 0.38268343236508977173};
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    Cplx v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = a[pidx(16 * q + 4 * g + k)];
    fft_regs<2, INV>(v);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[pidx(16 * q + 4 * g + k)] = v[k];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p0 = pidx(16 * q + j), p1 = pidx(16 * q + j + 4), p2 = pidx(16 * q + j + 8), p3 = pidx(16 * q + j + 12);
    const Cplx e0 = a[p0], e1 = a[p1], e2 = a[p2], e3 = a[p3];
    const Cplx w1 = {c16[2 * j], INV ? s16[2 * j] : -s16[2 * j]};  // W_8^j
    const Cplx wa = {c16[j], INV ? s16[j] : -s16[j]}, wb = {c16[j + 4], INV ? s16[j + 4] : -s16[j + 4]};
    const Cplx t1 = j == 0 ? e1 : cmul(e1, w1), t3 = j == 0 ? e3 : cmul(e3, w1);
    const Cplx f0 = cadd(e0, t1), f1 = csub(e0, t1), f2 = cadd(e2, t3), f3 = csub(e2, t3);
    const Cplx g2 = j == 0 ? f2 : cmul(f2, wa), g3 = cmul(f3, wb);
    a[p0] = cadd(f0, g2);
    a[p2] = csub(f0, g2);
    a[p1] = cadd(f1, g3);
    a[p3] = csub(f1, g3);
  }
}

// In-place FFT of the n elements at a[pidx(.)] (already in bit-reversed order).  INV: conjugated
// twiddles (no scaling).  First pass: radix 16 (radix 8 when log2 n is odd) in registers; then
// radix-4 passes.  tw: the per-pass tables described above (built by build_twiddles).
// SWEEPS: the radix-16 pass as fft16_two_sweeps.
template <bool INV, bool SWEEPS>
__device__ __forceinline__ void fft_inplace_body(Cplx *a, const Cplx *tw, int n, int logn, int tid) {
  int s0;
  if (logn < 3) {  // n = 2 or 4: plain radix-2 stages by one thread each
    for (int t = 0; t < logn; ++t) {
      const int h = 1 << t;
      for (int b = tid; b < n / 2; b += kFftThreads) {
        const int j = b & (h - 1), i0 = ((b >> t) << (t + 1)) | j;
        Cplx w = {1.0, 0.0};
        if (t == 1 && j == 1) w = {0.0, INV ? 1.0 : -1.0};
        const Cplx u = a[pidx(i0)], x = cmul(a[pidx(i0 + h)], w);
        a[pidx(i0)] = cadd(u, x);
        a[pidx(i0 + h)] = csub(u, x);
      }
      __syncthreads();
    }
    return;
  }
  if (logn & 1) {
    for (int q = tid; q < n / 8; q += kFftThreads) {
      Cplx v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = a[pidx(8 * q + k)];
      fft_regs<3, INV>(v);
#pragma unroll
      for (int k = 0; k < 8; ++k) a[pidx(8 * q + k)] = v[k];
    }
    s0 = 3;
  } else {
    for (int q = tid; q < n / 16; q += kFftThreads) {
      if (SWEEPS) {
        fft16_two_sweeps<INV>(a, q);
        continue;
      }
      Cplx v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = a[pidx(16 * q + k)];
      fft_regs<4, INV>(v);
#pragma unroll
      for (int k = 0; k < 16; ++k) a[pidx(16 * q + k)] = v[k];
    }
    s0 = 4;
  }
  __syncthreads();
  for (int s = s0; s < logn; s += 2) {  // stages s and s+1 in one pass
    const int h = 1 << s;
    const Cplx *tab = tw + tw_offset(s0, s);  // W_{4h}^j, j < 2h
    for (int q = tid; q < n / 4; q += kFftThreads) {
      const int j = q & (h - 1);
      const int base = ((q >> s) << (s + 2)) | j;
      const int p0 = pidx(base), p1 = pidx(base + h), p2 = pidx(base + 2 * h), p3 = pidx(base + 3 * h);
      Cplx e0 = a[p0], e1 = a[p1], e2 = a[p2], e3 = a[p3];
      Cplx w1 = tab[2 * j], wa = tab[j], wb = tab[j + h];  // W_{2h}^j = W_{4h}^{2j}
      if (INV) {
        w1.im = -w1.im;
        wa.im = -wa.im;
        wb.im = -wb.im;
      }
      const Cplx t1 = cmul(e1, w1), t3 = cmul(e3, w1);
      const Cplx f0 = cadd(e0, t1), f1 = csub(e0, t1), f2 = cadd(e2, t3), f3 = csub(e2, t3);
      const Cplx g2 = cmul(f2, wa), g3 = cmul(f3, wb);
      a[p0] = cadd(f0, g2);
      a[p2] = csub(f0, g2);
      a[p1] = cadd(f1, g3);
      a[p3] = csub(f1, g3);
    }
    __syncthreads();
  }
}

template <bool INV>
__device__ void fft_inplace(Cplx *a, const Cplx *tw, int n, int logn, int tid) {
  fft_inplace_body<INV, false>(a, tw, n, logn, tid);
}

// forward twiddles of every radix-4 pass of an n-point transform (see tw_offset); < n entries in total
__device__ void build_twiddles(Cplx *tw, int logn, int tid) {
  if (logn < 3) return;
  const int s0 = (logn & 1) ? 3 : 4;
  for (int s = s0; s < logn; s += 2) {
    const int h = 1 << s;
    Cplx *tab = tw + tw_offset(s0, s);
    for (int j = tid; j < 2 * h; j += kFftThreads) {
      double sn, cs;
      sincospi(-(double)j / (double)(2 * h), &sn, &cs);  // -2 pi j / (4h)
      tab[j] = {cs, sn};
    }
  }
}

__device__ __forceinline__ int bitrev(int i, int logn) { return (int)(__brev((unsigned)i) >> (32 - logn)); }

enum { kModeSpec = 0, kModeInverse = 1, kModeSmooth = 2, kModeBackward = 3 };

// spectra of the two packed real columns at bin k (0 <= k <= n/2) from Z_k and Z_{n-k}
__device__ __forceinline__ void unpack2(Cplx zk, Cplx zm, Cplx *x1, Cplx *x2) {
  *x1 = {0.5 * (zk.re + zm.re), 0.5 * (zk.im - zm.im)};
  *x2 = {0.5 * (zk.im + zm.im), 0.5 * (zm.re - zk.re)};
}
// Z_k and Z_{n-k} of z = h1 + i h2 for two HERMITIAN spectra given at bin k (their values at n-k are the conjugates)
__device__ __forceinline__ void pack2(Cplx h1, Cplx h2, Cplx *zk, Cplx *zm) {
  *zk = {h1.re - h2.im, h1.im + h2.re};
  *zm = {h1.re + h2.im, h2.re - h1.im};
}
__device__ __forceinline__ Cplx unit_phasor(Cplx s) {  // exp(i * angle(s)); numpy's angle(0) is 0
  const double mag = hypot(s.re, s.im);
  return mag > 0.0 ? Cplx{s.re / mag, s.im / mag} : Cplx{1.0, 0.0};
}

}  // namespace
}  // namespace mlpg

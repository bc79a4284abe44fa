// Strip MLPG kernels: the geometry that the kernels (mlpg_strip_impl.h) and the host-side dispatch (mlpg_strip.hip, capi.hip,
// streams_api.hip) must agree on -- sizes of a strip, of a record and of the control area, and the launchers' "nothing was
// enqueued" result.  Constants and constexpr arithmetic only: including it compiles no kernel.
#pragma once
#include <stddef.h>

#ifndef MLPG_STRIP_W
#define MLPG_STRIP_W 4   // 8: 128-frame strips, one workgroup of 8 wavefronts per CU (experiment)
#endif
#ifndef MLPG_STRIP_M
#define MLPG_STRIP_M 16  // 8: the 8-frame-chunk experiment of round 5 (profiles/r05_notes.md)
#endif

namespace mlpg {
namespace strip {

constexpr int kW = MLPG_STRIP_W;  // chunks (wavefronts) per strip (workgroup)
constexpr int kM = MLPG_STRIP_M;  // frames per chunk
constexpr int kFrames = kW * kM;  // frames per strip
constexpr int kRec = 14;          // doubles per lane in a level-1 / level-2 record
constexpr size_t kRecBytes = (size_t)kRec * 64 * 8;  // one strip's record in the scratch area: kRec doubles for each of 64 lanes

// Control words, one per 128-byte line (32 ints) so that the pollers of one utterance, the ticket draws and the
// arrivals of other utterances never queue on the same L2 line:
//   line 0: spin time-outs;  lines 1 .. 8: ticket of work list x;  line 9 + g: system group g -- word 0 arrivals,
//   words 2-3 mask of the lanes (systems) that met a failing pivot, word 4 time-out seen;
//   then one flag per strip, Rpad = R rounded up to a line per system group: flag[g * Rpad + r].
constexpr int kCtrlLine = 32;
constexpr int kMaxLists = 8;
constexpr int flag_pitch(int R) { return (R + kCtrlLine - 1) / kCtrlLine * kCtrlLine; }
constexpr size_t ctrl_ints(int nsg, int R) {
  return (size_t)(1 + kMaxLists + nsg) * kCtrlLine + (size_t)nsg * flag_pitch(R);
}
// Scratch layout for one launch: control words (ctrl_bytes), then the records (nsg * R * kRecBytes).
constexpr size_t ctrl_bytes(int nsg, int R) { return (ctrl_ints(nsg, R) * sizeof(int) + 255) / 256 * 256; }

constexpr int kNotResident = -1000;  // a launcher's result: the grid cannot hold an utterance's strips; nothing was enqueued

}  // namespace strip
}  // namespace mlpg

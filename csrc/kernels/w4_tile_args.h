// Host-side description of an MXFP4 LDS-tiled GEMM launch (mxfp4_gemm.hip w4a16_tile_kernel) and THE
// check that says whether the launch is taken.  Plain C++: no HIP, no torch.  The launcher calls
// w4t_takes before it enqueues anything, so a refusal (-1) always means "nothing launched, nothing
// written".  Operands and formats are those of w4_args.h; what differs is the row count (any M: the
// X tile of a k-chunk is staged in LDS once per workgroup) and the f32 workspace of the K split.
#pragma once
#include <stdint.h>

namespace mx {

constexpr int W4T_NC = 2;                          // 16-channel groups per wave
constexpr int W4T_NW = 4;                          // waves per workgroup: they split the channels
constexpr int W4T_BN = 16 * W4T_NC * W4T_NW;       // channels per workgroup
constexpr int W4T_CHUNK = 128;                     // k per pipeline stage: one LDS ring slot of X
constexpr int W4T_MAX_SPLIT = 4;                   // K parts over grid.z, at most
constexpr int W4T_FILL = 256;                      // workgroups wanted before K is left whole: the CUs
constexpr int64_t W4T_MAX_M = 65535 * 128;         // grid.y blocks of 128 rows

struct W4TileLaunch {
  const void* x;       // [M, K] bf16, row stride ldx (elements)
  int64_t ldx;
  const void* codes;   // [N, K/2] u8
  const void* scales;  // [N, K/32] u8
  void* y;             // [M, N] bf16, row stride ldy (elements)
  int64_t ldy;
  void* ws;            // f32 [w4t_splits, M, N] where w4t_splits > 1 (the K parts' partial sums), else unused
  int64_t M, N, K;
};

// 16-token MFMA blocks of a workgroup's M-block: 32, 64 or 128 rows; more rows go over grid.y.
inline int w4t_mblocks(int64_t M) { return M <= 32 ? 2 : M <= 64 ? 4 : 8; }

// K parts (grid.z).  A workgroup owns 128 channels, so the 70B o / down projections (N 8192) give 64
// workgroups for 256 CUs: K is split 2 or 4 ways until the grid fills the CUs, each part writes its f32
// partial sums to the workspace and a second kernel adds the parts in a fixed order.  K % 512 == 0
// keeps every part whole 128-k chunks.
inline int w4t_splits(int64_t M, int64_t N, int64_t K) {
  if (M < 1 || N < 1 || K < 1) return 1;
  const int64_t bm = 16 * w4t_mblocks(M);
  const int64_t wgs = ((N + W4T_BN - 1) / W4T_BN) * ((M + bm - 1) / bm);
  int s = 1;
  while (s < W4T_MAX_SPLIT && wgs * s < W4T_FILL) s *= 2;
  return s;
}

inline bool w4t_takes(const W4TileLaunch& L) {
  constexpr int64_t I32 = 0x7fffffff;
  // every pointer is dereferenced; the workspace only by a split launch
  if (!L.x || !L.codes || !L.scales || !L.y) return false;
  // grid.y blocks of 16 * w4t_mblocks rows
  if (L.M < 1 || L.M > W4T_MAX_M) return false;
  // whole 16-channel groups; a workgroup's channel numbers run up to N + W4T_BN - 1 as ints
  if (L.N < 16 || L.N % 16 || L.N > I32 - W4T_BN) return false;
  // every K part (1, 2 or 4 of them) is whole 128-k chunks
  if (L.K < 1 || L.K > I32 || L.K % (W4T_MAX_SPLIT * W4T_CHUNK)) return false;
  // X rows hold K elements and start 16-B aligned (16-B LDS-DMA pieces); Y rows hold N and start 16-B
  // aligned (8-B stores of four channels).  Row block starts, N * K / 2 and the workspace index are
  // formed in 64 bits.
  if (L.ldx < L.K || L.ldx % 8 || L.ldy < L.N || L.ldy % 8) return false;
  if ((uintptr_t)L.x % 16 || (uintptr_t)L.y % 16) return false;
  if ((uintptr_t)L.codes % 16 || (uintptr_t)L.scales % 4) return false;
  // the 32-bit byte offsets of the X buffer descriptor: row r < 128 of an M-block, byte
  // 2 * (r * ldx + k) + 16 <= 2 * (127 * ldx + K), which is also the descriptor's num_records
  if (L.ldx > (I32 / 2 - L.K) / 127) return false;
  if (w4t_splits(L.M, L.N, L.K) > 1 && (!L.ws || (uintptr_t)L.ws % 16)) return false;
  return true;
}

}  // namespace mx

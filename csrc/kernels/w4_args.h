// Host-side description of an MXFP4 weight-streaming decode GEMM launch (mxfp4_gemm.hip
// w4a16_gemm_kernel) and THE check that says whether the launch is taken.  Plain C++: no HIP, no
// torch -- the launcher, the torch binding and the stand-alone test (tests/native/test_w4_args.cpp)
// include this one file.  The launcher calls w4_takes before it enqueues anything, so a refusal (-1)
// always means "nothing launched, nothing written".
//
// Y[M, N] = X[M, K] . dequant(codes, scales)^T, OCP MXFP4 weights (mxllm/serve/quant.py):
//   codes  u8 [N, K/2]   two e2m1 codes per byte, the even k in the low nibble
//   scales u8 [N, K/32]  one e8m0 byte per 32 consecutive k of a channel
// both contiguous (a channel's row follows the previous one's), so only X and Y carry a row stride.
#pragma once
#include <stdint.h>

namespace mx {

constexpr int W4_MAX_M = 32;    // rows of one launch: two MFMA token blocks of 16
constexpr int W4_CHUNK = 128;   // k per lane-group step: a lane's 16-B code load is one 32-k block, x 4 groups
constexpr int W4_BLOCK = 32;    // k per scale byte

struct W4Launch {
  const void* x;       // [M, K] bf16, row stride ldx (elements)
  int64_t ldx;
  const void* codes;   // [N, K/2] u8
  const void* scales;  // [N, K/32] u8
  void* y;             // [M, N] bf16, row stride ldy (elements)
  int64_t ldy;
  int64_t M, N, K;
};

// The waves of a workgroup split K into that many contiguous parts, each whole 128-k chunks: eight
// where K allows it, four otherwise (K = 3584, a TP-8 shard of the 70B down projection, is 7 x 512).
// 0: no split fits, the launch is refused.
inline int w4_waves(int64_t K) {
  if (K <= 0) return 0;
  if (K % (8 * W4_CHUNK) == 0) return 8;
  if (K % (4 * W4_CHUNK) == 0) return 4;
  return 0;
}

// Whether the launch is taken (M >= 1: the launcher returns 0 for M <= 0 before it asks).
inline bool w4_takes(const W4Launch& L) {
  constexpr int64_t I32 = 0x7fffffff;
  // every pointer is dereferenced
  if (!L.x || !L.codes || !L.scales || !L.y) return false;
  // one or two 16-token MFMA blocks
  if (L.M < 1 || L.M > W4_MAX_M) return false;
  // whole 16-channel groups; N / 16 workgroups at most (grid.x), N and K are ints in the kernel
  if (L.N < 16 || L.N % 16 || L.N > I32) return false;
  // each wave's K part is whole 128-k chunks
  if (L.K > I32 || !w4_waves(L.K)) return false;
  // X rows hold K elements and start 16-B aligned (16-B fragment loads); Y rows hold N and start
  // 16-B aligned (8-B stores of four channels).  M * ldx, N * K / 2 are formed in 64 bits.
  if (L.ldx < L.K || L.ldx % 8 || L.ldy < L.N || L.ldy % 8) return false;
  if ((uintptr_t)L.x % 16 || (uintptr_t)L.y % 16) return false;
  // code rows are K / 2 bytes, a multiple of 256: 16-B loads need the base aligned; a wave's scale
  // word (the four bytes of a chunk) needs the scale base 4-B aligned
  if ((uintptr_t)L.codes % 16 || (uintptr_t)L.scales % 4) return false;
  return true;
}

}  // namespace mx

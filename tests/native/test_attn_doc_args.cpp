// Stand-alone check of mx::ad_takes (csrc/kernels/attn_doc_args.h), host compile only: a launcher in the
// launcher's shape -- ask the check, then count what would be enqueued -- must count nothing for every
// refused description and something for the taken ones.  Addresses are integers, never dereferenced.
#include "kernels/attn_doc_args.h"

#include <cstdio>
#include <initializer_list>

using namespace mx;

static int launched = 0;
static int launch(const AdLaunch& L) {  // mx_attn_doc's order: the check first, then the kernels
  if (!ad_takes(L)) return -1;
  if (ad_empty(L)) return 0;
  launched += L.bwd ? 3 : 1;
  return 0;
}

static AdLaunch good(int bwd) {
  AdLaunch L{};
  void* p = reinterpret_cast<void*>((uintptr_t)0x1000);
  L.bwd = bwd;
  L.q = L.k = L.v = L.doc_start = p, L.o = L.lse = p;
  L.q_bf16 = L.kv_bf16 = L.o_bf16 = L.lse_f32 = L.doc_i32 = 1;
  L.B = 2, L.Hq = 8, L.Hkv = 2, L.S = 257, L.D = 128, L.ldo = 8 * 128 + 16;
  if (bwd) {
    L.doc_end = L.dout = p, L.delta = L.dq = L.dkp = L.dvp = L.work = p;
    L.dout_bf16 = L.out_f32 = 1;
  }
  return L;
}

static int fails = 0;
static void expect(const char* what, const AdLaunch& L, int rc, int n) {
  const int before = launched, got = launch(L);
  if (got != rc || launched - before != n) {
    printf("FAIL %s: rc %d (want %d), launched %d (want %d)\n", what, got, rc, launched - before, n);
    ++fails;
  }
}

int main() {
  for (int bwd = 0; bwd < 2; ++bwd) {
    const int n = bwd ? 3 : 1;
    AdLaunch L = good(bwd);
    expect("taken", L, 0, n);
    for (int64_t D : {32, 64}) { L = good(bwd); L.D = D; L.ldo = L.Hq * D; expect("D 32 / 64", L, 0, n); }
    L = good(bwd); L.B = 0; expect("empty batch", L, 0, 0);
    L = good(bwd); L.S = 0; expect("empty sequence", L, 0, 0);
    L = good(bwd); L.doc_start = nullptr; expect("no doc_start", L, -1, 0);
    L = good(bwd); L.doc_i32 = 0; expect("tables not int32", L, -1, 0);
    L = good(bwd); L.D = 96; expect("D 96", L, -1, 0);
    L = good(bwd); L.Hkv = 3; expect("Hq % Hkv", L, -1, 0);
    L = good(bwd); L.ldo = L.Hq * L.D - 8; expect("ldo below the row", L, -1, 0);
    L = good(bwd); L.ldo += 4; expect("ldo % 8", L, -1, 0);
    L = good(bwd); L.q_bf16 = 0; expect("q not bf16", L, -1, 0);
    L = good(bwd); L.k = nullptr; expect("no k", L, -1, 0);
    L = good(bwd); L.o = nullptr; expect("no o", L, -1, 0);
    L = good(bwd); L.B = 1 << 20, L.S = 1 << 20; expect("rows past 31 bits", L, -1, 0);
    L = good(bwd); L.bwd = 2; expect("bad direction", L, -1, 0);
  }
  AdLaunch L = good(1);
  L.doc_end = nullptr; expect("backward without doc_end", L, -1, 0);
  L = good(1); L.work = nullptr; expect("backward without the dS^T image", L, -1, 0);
  L = good(1); L.dq = nullptr; expect("backward without dq", L, -1, 0);
  L = good(1); L.out_f32 = 0; expect("backward outputs not f32", L, -1, 0);
  L = good(1);
  if (ad_work_bytes(L) != 2 * 8 * (3 * 128) * 320 * 2) { printf("FAIL ad_work_bytes %lld\n", (long long)ad_work_bytes(L)); ++fails; }
  printf("%s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}

// Stand-alone driver of mx::pp8_takes (csrc/kernels/prefill_paged_kv8_args.h): reads launches from stdin as
// whitespace-separated integers -- q o bt segs work (addresses, never dereferenced) q_bf16 o_bf16 T Hq D slots
// maxb ldo nwork (-1: pp_work_count of the segments) nseg, then row0 n slot p0 per segment, then for each of
// k_codes k_scale v_codes v_scale: address dtype_ok contiguous ndim (<= 4) and ndim sizes -- and prints
// pp8_takes per launch.  tests/test_prefill_paged_kv8_args.py builds it plain and under ASan + UBSan.
#include "kernels/prefill_paged_kv8_args.h"

#include <iostream>

using namespace mx;

int main() {
  long long q, o, bt, segs, work, nwork, nseg;
  PpKv8Launch L{};
  while (std::cin >> q >> o >> bt >> segs >> work >> L.q_bf16 >> L.o_bf16 >> L.T >> L.Hq >> L.D >> L.slots >> L.maxb >>
         L.ldo >> nwork >> nseg) {
    std::vector<PpSeg> sg((size_t)nseg);
    for (PpSeg& s : sg) std::cin >> s.row0 >> s.n >> s.slot >> s.p0;
    for (Pp8Pool* p : {&L.k_codes, &L.k_scale, &L.v_codes, &L.v_scale}) {
      long long a;
      *p = Pp8Pool{};
      std::cin >> a >> p->dtype_ok >> p->contiguous >> p->ndim;
      p->p = reinterpret_cast<void*>((uintptr_t)a);
      for (int d = 0; d < p->ndim && d < 4; ++d) std::cin >> p->dim[d];
    }
    L.q = reinterpret_cast<void*>((uintptr_t)q), L.o = reinterpret_cast<void*>((uintptr_t)o);
    L.bt = reinterpret_cast<const int32_t*>((uintptr_t)bt), L.segs = reinterpret_cast<const int32_t*>((uintptr_t)segs);
    L.work = reinterpret_cast<const int32_t*>((uintptr_t)work);
    L.nseg = nseg, L.segs_host = sg.empty() ? nullptr : sg.data();
    L.nwork = nwork < 0 ? pp_work_count(sg.data(), nseg) : nwork;
    std::cout << (pp8_takes(L) ? 1 : 0) << "\n";
  }
  return 0;
}

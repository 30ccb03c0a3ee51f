// Stand-alone driver of mx::w4_takes (csrc/kernels/w4_args.h), the one operand check of the MXFP4
// decode GEMM launcher: reads one launch description per line from stdin -- `key=value` tokens,
// integers in any base strtoll takes, addresses as integers (never dereferenced), missing keys 0 --
// and prints per line `<w4_takes> <w4_waves(K)> <last byte offsets>`: 1 (taken) or 0 (refused), the
// number of K-splitting waves, and -- for a taken launch -- the offsets of the last byte the kernel
// reads of x, codes and scales and writes of y, formed as the kernel forms them (64-bit), so that a
// wrap would show as a sanitizer report or a wrong number.  tests/test_w4_args.py builds this file
// plain and under AddressSanitizer + UBSan.
#include "kernels/w4_args.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace mx;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    W4Launch L{};
    std::istringstream ss(line);
    std::string tok;
    while (ss >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        fprintf(stderr, "bad token %s\n", tok.c_str());
        return 2;
      }
      const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
      const long long i = strtoll(v.c_str(), nullptr, 0);
      void* p = reinterpret_cast<void*>((uintptr_t)strtoull(v.c_str(), nullptr, 0));
      if (k == "x") L.x = p;
      else if (k == "ldx") L.ldx = i;
      else if (k == "codes") L.codes = p;
      else if (k == "scales") L.scales = p;
      else if (k == "y") L.y = p;
      else if (k == "ldy") L.ldy = i;
      else if (k == "M") L.M = i;
      else if (k == "N") L.N = i;
      else if (k == "K") L.K = i;
      else {
        fprintf(stderr, "unknown key %s\n", k.c_str());
        return 2;
      }
    }
    const bool ok = w4_takes(L);
    long long x_end = 0, q_end = 0, s_end = 0, y_end = 0;
    if (ok) {  // only then are these products known to fit
      x_end = 2 * ((L.M - 1) * L.ldx + L.K);
      q_end = (L.N - 1) * (L.K / 2) + L.K / 2;
      s_end = (L.N - 1) * (L.K / 32) + L.K / 32;
      y_end = 2 * ((L.M - 1) * L.ldy + L.N);
    }
    printf("%d %d %lld %lld %lld %lld\n", ok ? 1 : 0, w4_waves(L.K), x_end, q_end, s_end, y_end);
  }
  return 0;
}

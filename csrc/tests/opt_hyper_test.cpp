// Host test of csrc/include/psamd_opt_hyper.h (built and run by tests/test_opt_hyper_cpu.py under
// the address and undefined-behaviour sanitizers).  Prints
//   names <the 16 field names in order>
//   bias <mode> <step> <bits of bc1> <bits of bc2>     betas 0.9 / 0.999, bc1 / bc2 3 / 5 before
// and exits non-zero when the decode of 1..16 puts a value in the wrong field or a vector of 15
// is not refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "psamd_opt_hyper.h"

static int failures = 0;
#define EXPECT(cond)                        \
  if (!(cond)) {                            \
    std::printf("FAILED: %s\n", #cond);     \
    ++failures;                             \
  }

static unsigned bits(float x) {
  unsigned u;
  std::memcpy(&u, &x, sizeof(u));
  return u;
}

static double& at(std::vector<double>& v, const char* name) {
  for (int i = 0; i < psamd::kOptHyperLen; ++i)
    if (std::strcmp(psamd::kOptHyperNames[i], name) == 0) return v[static_cast<size_t>(i)];
  std::printf("FAILED: no field %s\n", name);
  std::exit(1);
}

int main() {
  using namespace psamd;
  std::printf("names");
  for (const char* name : kOptHyperNames) std::printf(" %s", name);
  std::printf("\n");

  std::vector<double> v(kOptHyperLen);
  for (int i = 0; i < kOptHyperLen; ++i) v[static_cast<size_t>(i)] = i + 1;
  at(v, "adamw") = 0.0;  // the 9th; nesterov (8.0) is on
  const OptHyper h = opt_hyper_decode(v);
  EXPECT(h.lr == 1.f && h.beta1 == 2.f && h.beta2 == 3.f && h.eps == 4.f && h.wd == 5.f);
  EXPECT(h.momentum == 6.f && h.dampening == 7.f && h.nesterov == 1 && h.adamw == 0);
  EXPECT(h.bc1 == 10.f && h.bc2 == 11.f && h.l1 == 12.f && h.l2 == 13.f && h.fbeta == 14.f);
  EXPECT(h.ftrl_mode == 15 && h.gscale == 16.f);

  bool threw = false;
  try {
    v.pop_back();
    (void)opt_hyper_decode(v);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);

  v.assign(kOptHyperLen, 0.0);
  at(v, "beta1") = 0.9, at(v, "beta2") = 0.999, at(v, "bc1") = 3.0, at(v, "bc2") = 5.0;
  for (int mode = 0; mode < 3; ++mode)
    for (int64_t step : {1, 2, 1000}) {
      OptHyper b = opt_hyper_decode(v);
      opt_bias_correct(b, mode, step);
      std::printf("bias %d %lld %08x %08x\n", mode, static_cast<long long>(step), bits(b.bc1), bits(b.bc2));
    }
  return failures == 0 ? 0 : 1;
}

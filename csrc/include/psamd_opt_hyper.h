// The optimizer hyper-parameter record of every opt_apply<KIND> caller (csrc/kernels/optim.hip).
//
// Python packs the record as a flat list of doubles (ps_amd/ops/optim.py hyper_vec, checked
// against kOptHyperNames when the extension loads); the bindings and the native engines unpack
// it with opt_hyper_decode.  The field order is written here and nowhere else in C++.  No HIP
// and no torch in this header: csrc/tests/opt_hyper_test.cpp builds it with a host compiler.
#pragma once
#include <stdint.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

namespace psamd {

struct OptHyper {
  float lr, beta1, beta2, eps, wd, momentum, dampening;
  int nesterov, adamw;
  float bc1, bc2;  // multipliers of adam's m and v (bias correction), host-computed
  float l1, l2, fbeta;
  int ftrl_mode;  // 0 canonical, 1 reference
  float gscale;   // host gradient multiplier
};

constexpr int kOptHyperLen = 16;
const char* const kOptHyperNames[kOptHyperLen] = {"lr",        "beta1",    "beta2", "eps", "wd", "momentum",
                                                  "dampening", "nesterov", "adamw", "bc1", "bc2", "l1",
                                                  "l2",        "fbeta",    "ftrl_mode", "gscale"};

inline OptHyper opt_hyper_decode(const std::vector<double>& v) {
  if (v.size() != static_cast<size_t>(kOptHyperLen))
    throw std::invalid_argument("optimizer hyper-parameters: " + std::to_string(kOptHyperLen) + " values, got " +
                                std::to_string(v.size()));
  const auto f = [&](int i) { return static_cast<float>(v[static_cast<size_t>(i)]); };
  const auto flag = [&](int i) { return v[static_cast<size_t>(i)] != 0.0 ? 1 : 0; };
  OptHyper h;
  h.lr = f(0); h.beta1 = f(1); h.beta2 = f(2); h.eps = f(3); h.wd = f(4); h.momentum = f(5); h.dampening = f(6);
  h.nesterov = flag(7); h.adamw = flag(8); h.bc1 = f(9); h.bc2 = f(10);
  h.l1 = f(11); h.l2 = f(12); h.fbeta = f(13); h.ftrl_mode = static_cast<int>(v[14]); h.gscale = f(15);
  return h;
}

// Adam's bias correction as the asynchronous engines apply it per served push.  bias_mode 0: bc1 /
// bc2 as decoded; 1: 1 / (1 - beta^step), in double on the float betas; 2: the reference's
// constant 1 / (1 - beta), in float.
inline void opt_bias_correct(OptHyper& h, int bias_mode, int64_t step) {
  if (bias_mode == 1) {
    const auto bc = [step](float beta) {
      return static_cast<float>(1.0 / (1.0 - std::pow(static_cast<double>(beta), static_cast<double>(step))));
    };
    h.bc1 = bc(h.beta1);
    h.bc2 = bc(h.beta2);
  } else if (bias_mode == 2) {
    h.bc1 = 1.f / (1.f - h.beta1);
    h.bc2 = 1.f / (1.f - h.beta2);
  }
}

constexpr bool opt_kind_valid(int64_t kind) { return kind >= 0 && kind <= 3; }  // sgd adam adagrad ftrl

}  // namespace psamd

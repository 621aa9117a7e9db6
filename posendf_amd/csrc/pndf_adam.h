// The ONE Adam of the library: torch.optim.Adam (no amsgrad) as torch's _single_tensor_adam runs it, shared by pndf_adam_step_kernel
// (pndf_optim.hip: the trainer's flat parameter buffer, coupled L2 weight decay) and pndf_denoise_update_kernel (pndf_denoise.hip:
// the poses of the motion-denoise and image-fitting loops, weight decay 0).  The scalars are formed on the host as torch forms them --
// Python floats, i.e. double -- and each is rounded ONCE to fp32 where it meets the tensors; the device does no transcendental and
// no subtraction of nearly equal fp32 constants (1.0f - 0.999f is 1.3e-5 away from 0.001).
#pragma once
#include <cmath>

struct AdamScalars {
    float one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps, weight_decay;
};
static_assert(sizeof(AdamScalars) == 28, "AdamScalars layout");

// step >= 1; lr / (1 - beta1^step) and sqrt(1 - beta2^step) in double
inline AdamScalars pndf_adam_scalars(int step, double lr, double beta1, double beta2, double eps, double weight_decay) {
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    AdamScalars s;
    s.one_minus_beta1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.one_minus_beta2 = (float)(1.0 - beta2);
    s.step_size = (float)(lr / bc1);
    s.bc2_sqrt = (float)std::sqrt(bc2);
    s.eps = (float)eps;
    s.weight_decay = (float)weight_decay;
    return s;
}

#ifdef __HIPCC__
// one element of torch's _single_tensor_adam, in its order of operations
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamScalars& s) {
    g = g + s.weight_decay * p;                        // grad.add(param, alpha=weight_decay)
    m = m + s.one_minus_beta1 * (g - m);               // exp_avg.lerp_(grad, 1 - beta1)
    v = v * s.beta2 + s.one_minus_beta2 * (g * g);     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps; // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - s.step_size * (m / denom);                 // param.addcdiv_(exp_avg, denom, value=-step_size)
}
#endif

// mh_phase_grad.hpp — the derivative of the Henyey-Greenstein phase function
// with respect to its asymmetry g (host and device).
//
// eval_hg's conventions (mh_shading.hpp, phase/hg.cpp:66-72): cos_theta is the
// cosine handed to eval_hg (-wo.z of the local outgoing direction) and
//   temp = 1 + g^2 + 2 g cos_theta,   p = (1 - g^2) / (4 pi temp^(3/2)).
// Then  d ln p / d g = -2 g / (1 - g^2) - 3 (g + cos_theta) / temp:
// no division by g, and -3 cos_theta at g = 0.  The prbvolpath adjoint charges
// it at every real scatter event of an `hg` medium (prbvol_sample's PhG
// instances), mh_phase_eval_grad returns p times it, and
// tools/phase_g_check.cpp checks it on the host against central differences.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MH_PG_FN __host__ __device__ inline
#else
#define MH_PG_FN inline
#endif

namespace mh {

MH_PG_FN float hg_dlog_dg(float g, float cos_theta) {
    const float temp = (1.f + g * g) + (2.f * g) * cos_theta;
    return (-2.f * g) / (1.f - g * g) - (3.f * (g + cos_theta)) / temp;
}

}  // namespace mh

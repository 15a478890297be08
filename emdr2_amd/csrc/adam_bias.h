// emdr2_amd/csrc/adam_bias.h -- Adam's bias corrections, stated once for the entries that apply the update (optimizer.hip) and the one that
// reports it (param_stats.hip): host fp32, bc = 1 - powf(beta, (float)step).  The kernels receive the two floats as arguments.
#ifndef EMDR2_ADAM_BIAS_H
#define EMDR2_ADAM_BIAS_H
#include <math.h>

static inline void adam_bias_corrections(float beta1, float beta2, int step, float *bc1, float *bc2)
{
    *bc1 = 1.f - powf(beta1, (float)step);
    *bc2 = 1.f - powf(beta2, (float)step);
}
#endif

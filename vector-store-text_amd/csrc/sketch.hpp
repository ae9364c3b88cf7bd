// sketch.hpp — the per-row int8 sketch of an f32 row and the bound that lets the
// register search reject a candidate without reading its f32 row.
//
// Row x (dim f32 elements) -> u[i] = rint(x[i] / scale) + 128 (one byte each),
// scale = max|x[i]| / 127, i.e. x~[i] = scale * (u[i] - 128), and one number
//     err >= |x - x~|_2 + slack.
// For any query q, Cauchy-Schwarz gives |q.x - q.x~| <= |q| |x - x~|, so
//     q.x <= q.x~ + |q| err,   and   1 - (q.x~ + |q| err)
// is a lower bound of the dot-metric distance 1 - q.x.
//
// The search compares that bound with the distance the exact kernel would have
// computed in f32, and computes the bound itself in f32, so `err` also carries
// the rounding of both sums (u = 2^-24, every term of a d-term f32 sum of
// products passes through at most d roundings, whatever the order and with or
// without FMA: |fl(sum a_i b_i) - sum a_i b_i| <= g_d sum |a_i b_i|,
// g_d = d u / (1 - d u)):
//   exact sum   fl(q.x): error <= g_d sum |q_i x_i| <= g_d |q| |x|;
//   sketch sum  s = fl(sum q_i u_i), u_i <= 255: error <= g_d 255 |q|_1
//               <= g_d 255 sqrt(d) |q|;
//   bias        128 fl(sum q_i): error <= 128 g_d sqrt(d) |q|;
//   t = fl(s - 128 sum q), fl(scale t), the FMA with |q| err: three roundings
//               of values bounded by |q| (|x| + 2 err) (|scale t| ~ |q.x~|).
// Divided by |q| and rounded up generously (d + 8 for d, 384 for 255 + 128,
// 1.01 for the 1 / (1 - d u) factors; |x| <= sqrt(d) max|x_i| = 127 sqrt(d) scale):
//     slack = (d + 8) u 1.01 * (384 sqrt(d) scale + |x|_up + 2 e) + 4 u (|x|_up + 2 e),
// of the order of dim 2^-24 (|x| + 384 sqrt(dim) scale): 3e-4 for a unit 768-d
// row against e ~ 8e-3.  e itself is a f32 sum of squares of residuals each
// computed with one rounding (FMA), so it is inflated by (1 + (d + 8) 2^-23)
// before the slack is added.  The kernel multiplies err by an upper bound of
// |q| (its f32 norm inflated the same way).
//
// err = +inf (never rejected) for a row with a non-finite element, an all-zero
// row, a scale that is not a normal float or whose reciprocal overflows.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSG_HD __host__ __device__
#else
#define VSG_HD
#endif

namespace vsg {

struct SketchMeta {
    float scale;
    float err;
};

// sketch row stride: the u8 row starts 128-B aligned
static inline VSG_HD size_t sketch_stride(int dim) { return ((size_t)dim + 127) / 128 * 128; }

// max |x_i| of a row; NaN / inf propagate as +inf
static inline VSG_HD float sketch_maxabs(const float* x, int dim) {
    float m = 0.f;
    for (int i = 0; i < dim; ++i) {
        const float a = fabsf(x[i]);
        if (!(a <= 3.4028234e38f)) return INFINITY;  // NaN or inf
        m = a > m ? a : m;
    }
    return m;
}

// scale of a row with that max |x_i|; 0 = the row gets no usable sketch
static inline VSG_HD float sketch_scale(float maxabs) {
    // normal, and small enough that x / scale and 127 sqrt(d) scale stay finite
    if (!(maxabs >= 1e-30f) || !(maxabs <= 1e30f)) return 0.f;
    return maxabs / 127.f;
}

static inline VSG_HD uint8_t sketch_quant(float x, float scale) {
    float k = rintf(x / scale);
    k = k > 127.f ? 127.f : (k < -127.f ? -127.f : k);
    return (uint8_t)((int)k + 128);
}

// squared residual of one element: (x - scale (u - 128))^2, the residual with one rounding
static inline VSG_HD float sketch_res2(float x, float scale, uint8_t u) {
    const float r = fmaf(-scale, (float)((int)u - 128), x);
    return r * r;
}

// err from the f32 sums sum_res2 = sum (x_i - x~_i)^2 and sum_x2 = sum x_i^2 (any order)
static inline VSG_HD float sketch_err(float sum_res2, float sum_x2, float scale, int dim) {
    if (!(scale > 0.f)) return INFINITY;
    const float u = 5.9604645e-8f;  // 2^-24
    const float infl = 1.f + (float)(dim + 8) * 2.f * u;
    const float e = sqrtf(sum_res2) * infl;
    const float xn = sqrtf(sum_x2) * infl;
    const float sd = sqrtf((float)dim) * 1.0001f;
    const float mag = xn + 2.f * e;
    const float slack = (float)(dim + 8) * u * 1.01f * (384.f * sd * scale + mag) + 4.f * u * mag;
    const float r = (e + slack) * (1.f + 8.f * u);  // the roundings of this function
    return r == r ? r : INFINITY;
}

// Whole row at once (host tests; the device kernel computes the same values
// with the reductions spread over a wave).  out: sketch_stride(dim) bytes,
// padding = 128 (x~ = 0).
static inline VSG_HD SketchMeta sketch_row(const float* x, int dim, uint8_t* out) {
    const size_t stride = sketch_stride(dim);
    SketchMeta m;
    m.scale = sketch_scale(sketch_maxabs(x, dim));
    if (!(m.scale > 0.f)) {
        for (size_t i = 0; i < stride; ++i) out[i] = 128;
        m.scale = 0.f;
        m.err = INFINITY;
        return m;
    }
    float r2 = 0.f, x2 = 0.f;
    for (int i = 0; i < dim; ++i) {
        out[i] = sketch_quant(x[i], m.scale);
        r2 += sketch_res2(x[i], m.scale, out[i]);
        x2 = fmaf(x[i], x[i], x2);
    }
    for (size_t i = (size_t)dim; i < stride; ++i) out[i] = 128;
    m.err = sketch_err(r2, x2, m.scale, dim);
    if (!(m.err < INFINITY)) m.scale = 0.f;
    return m;
}

// upper bound of |q|_2 from the f32 sum of squares
static inline VSG_HD float sketch_qnorm_up(float sum_q2, int dim) {
    return sqrtf(sum_q2) * (1.f + (float)(dim + 8) * 1.1920929e-7f);
}

}  // namespace vsg

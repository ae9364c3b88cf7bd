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
//   sketch side: budgeted as g_d 384 sqrt(d) |q| scale plus three roundings of values
//               bounded by |q| (|x| + 2 err) -- the f32 sums of the first kernel
//               (fl(sum q_i u_i) and its bias 128 fl(sum q_i)); the integer sketch pass
//               below spends less.
// Divided by |q| and rounded up generously (d + 8 for d, 1.01 for the 1 / (1 - d u)
// factors; |x| <= sqrt(d) max|x_i| = 127 sqrt(d) scale):
//     slack = (d + 8) u 1.01 * (384 sqrt(d) scale + |x|_up + 2 e) + 4 u (|x|_up + 2 e),
// of the order of dim 2^-24 (|x| + 384 sqrt(dim) scale): 3e-4 for a unit 768-d
// row against e ~ 8e-3.  e itself is a f32 sum of squares of residuals each
// computed with one rounding (FMA), so it is inflated by (1 + (d + 8) 2^-23)
// before the slack is added.  The kernel multiplies err by an upper bound of
// |q| (its f32 norm inflated the same way).
//
// The sketch pass itself is integer (sketch_device.hpp).  Per search the query is
// quantised to 16 bits, q16_i = rint(q_i / s_q), s_q = max|q_i| / 32512, held as two
// signed int8 planes q16 = 256 h + l (h in [-127, 127], l in [-128, 127]); a row's signed
// bytes are x'_i = u_i - 128 (u ^ 0x80).  With q^ = s_q q16 (real numbers),
//     q.x = q^.x~ + (q - q^).x~ + q.(x - x~),
//     q^.x~ = s_q scale (256 H + L),  H = sum x'_i h_i,  L = sum x'_i l_i,
// H and L exact in int32 (|H|, |L| <= 127 128 d < 2^31 up to 8 KiB rows and far beyond),
//     |(q - q^).x~| <= qerr |x~| <= qerr 127 sqrt(d) scale,  qerr >= |q - q^|_2,
//     |q.(x - x~)| <= |q| e.
// The kernel evaluates (sketch_upper)
//     ub = fma(p, S, fma(qe, scale, fl(qn err))),  p = fl(s_q scale),
//     S = fma(256, fl(H), fl(L)),  qe = qerr 127 sqrt(d) 1.001.
// Its roundings: fl(H), fl(L) (inexact only above 2^24, d > 1040) and S's fma, each
// relative u of at most 256 |H| + |L| <= sum |x'_i| (|q16_i| + 256)
// <= 127 sqrt(d) (|q16| + 256 sqrt(d)); times p, and s_q 256 sqrt(d) <= |q| sqrt(d) / 127:
//     p |S - (256 H + L)| <= 3.03 u (1 + sqrt(d) / 127) 127 sqrt(d) scale |q|
//                         <= (385 + 3.1 sqrt(d)) u sqrt(d) scale |q|,
// below the (d + 8) u 1.01 * 384 sqrt(d) scale |q| that err holds for the f32 sketch sums
// (388 (d + 8) > 385 + 3.1 sqrt(d) for every d).  p, fl(qn err) and the two fmas are four
// roundings: of |p S| <= |q| (|x| + e) twice, of qn err three times (err < 0.52 (|x|_up +
// 2 e): e <= (|x|_up + 2 e) / 2, slack < 0.02 of it), of qe scale twice -- 3.7 u |q| (|x|_up
// + 2 e), inside err's 4 u (|x|_up + 2 e), and the 2 u qe scale inside qe's factor 1.001.
// So no row's err is loosened; the query pays qe scale, 1-2e-4 for a unit 768-d query
// against |q| err ~ 8e-3.  Underflow: the query is filtered only for max|q_i| in
// [2^-40, 2^40] and a row rejected only for p >= 2^-80, where p, p S and qn err are
// normal floats; qe scale >= 0 can only lose 2^-149 to it, and qerr carries 2^-40 max|q_i|
// for the squares of residuals that underflowed.
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

// ---- the query side: 16-bit quantisation in two signed int8 planes ----

// s_q of a query with that max |q_i|; 0 = the query runs unfiltered (all-zero,
// non-finite, or outside [2^-40, 2^40]: inside, s_q, 1 / s_q and |q| are normal floats
// far from both ends of the range)
static inline VSG_HD float sketch_qscale(float maxabs) {
    if (!(maxabs >= 9.094947e-13f) || !(maxabs <= 1.0995116e12f)) return 0.f;
    return maxabs / 32512.f;
}

// q16 = rint(q / s_q), |q16| <= 32512
static inline VSG_HD int sketch_q16(float q, float sq) {
    float k = rintf(q / sq);
    k = k > 32512.f ? 32512.f : (k < -32512.f ? -32512.f : k);
    return (int)k;
}
// q16 = 256 h + l: h = floor((q16 + 128) / 256) in [-127, 127], l in [-128, 127]
static inline VSG_HD int sketch_q16_hi(int q16) { return (q16 + 32768 + 128) / 256 - 128; }
static inline VSG_HD int sketch_q16_lo(int q16) { return q16 - 256 * sketch_q16_hi(q16); }

// squared residual of one element: (q - s_q q16)^2, the residual with one rounding
static inline VSG_HD float sketch_qres2(float q, float sq, int q16) {
    const float r = fmaf(-sq, (float)q16, q);
    return r * r;
}

// What a search keeps of its query: sq = s_q (0 = no filter), qe = the query's share of the
// bound per unit of a row's scale (qerr 127 sqrt(d), rounded up), qn >= |q|.
struct SketchQuery {
    float sq, qe, qn;
};

// from max |q_i| and the f32 sums sum_res2 = sum (q_i - s_q q16_i)^2 and sum_q2 = sum q_i^2
// (any order)
static inline VSG_HD SketchQuery sketch_query(float maxabs, float sum_res2, float sum_q2, int dim) {
    SketchQuery r;
    r.sq = sketch_qscale(maxabs);
    r.qn = sketch_qnorm_up(sum_q2, dim);
    const float infl = 1.f + (float)(dim + 8) * 1.1920929e-7f;
    // + 2^-40 max|q|: above anything the squares lost to underflow
    const float qerr = sqrtf(sum_res2) * infl + 9.094947e-13f * maxabs;
    r.qe = qerr * (127.f * sqrtf((float)dim)) * 1.001f;
    if (!(r.qe < INFINITY) || !(r.qn < INFINITY)) r.sq = 0.f;
    return r;
}

// smallest s_q * scale a row is rejected on (2^-80): the product p and p S are normal
// floats above it, and qn err >= 2^11 p
#define VSG_SKETCH_PMIN 8.2718061e-25f

// The upper bound of q . x in the kernel's own f32 arithmetic, from the integer sums
// H = sum x'_i h_i and L = sum x'_i l_i (x' = u - 128).  +inf / NaN: not rejected.
static inline VSG_HD float sketch_upper(const SketchQuery& q, SketchMeta m, int H, int L) {
    const float p = q.sq * m.scale;
    const float S = fmaf(256.f, (float)H, (float)L);
    const float ub = fmaf(p, S, fmaf(q.qe, m.scale, q.qn * m.err));
    return p >= VSG_SKETCH_PMIN ? ub : INFINITY;
}

// ---- the estimate itself: the walk distance of the int8 traversal ----

// A row's sketch can be evaluated: both meta words finite and the scale positive.  Not so
// for an all-zero or non-finite row (scale 0, err +inf) and for a row not converted yet
// (meta words all ones: NaN) -- such a row is scored from its f32 row.
static inline VSG_HD bool sketch_usable(SketchMeta m) {
    return m.scale > 0.f && m.scale <= 3.4028234e38f && m.err <= 3.4028234e38f;
}

// q . x~ in the kernel's f32 arithmetic from the integer sums H and L of sketch_upper,
// without its error terms: fl(s_q scale) * fma(256, fl(H), fl(L)).  On integer data in
// [-127, 127] with an element of magnitude 127 on both sides (scale 1, s_q 2^-8, l = 0) and
// 127^2 d < 2^24 (d <= 1040; stated for d <= 520) every step is exact: the estimate is q . x.
static inline VSG_HD float sketch_estimate(const SketchQuery& q, SketchMeta m, int H, int L) {
    const float p = q.sq * m.scale;
    return p * fmaf(256.f, (float)H, (float)L);
}

// The metric distance of an estimate: 1 - est (ip, cos), |x|^2 + |q|^2 - 2 est (l2sq; xn =
// the stored |x|^2, qn = |q|^2 summed once per query).  Exact whenever its terms are integers
// below 2^24.
static inline VSG_HD float sketch_dist_dot(float est) { return 1.f - est; }
static inline VSG_HD float sketch_dist_l2(float est, float xn, float qn) { return fmaf(-2.f, est, xn + qn); }

}  // namespace vsg

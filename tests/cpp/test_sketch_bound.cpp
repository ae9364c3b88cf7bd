// The int8 sketch of csrc/sketch.hpp on the CPU: for random, heavy-tailed, denormal,
// all-zero and non-finite rows and 1,000 random unit queries each, checked in f64:
//   |q.x - q.x~| <= err   (x~ = scale * (u - 128), the value the bytes stand for),
// and, with the sums done in f32 the way the kernels do them, that the sketch's lower
// bound never exceeds the f32 distance of the exact pass;
// rows with a non-finite element (and all-zero rows) get err = +inf.
// Stand-alone: g++ -fsanitize=address,undefined tests/cpp/test_sketch_bound.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../vector-store-text_amd/csrc/sketch.hpp"

using vsg::SketchMeta;

static int g_fail = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (g_fail < 20) {                    \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);         \
                std::printf("\n");                \
            }                                     \
            ++g_fail;                             \
        }                                         \
    } while (0)

static std::vector<std::vector<float>> unit_queries(int dim, int n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<std::vector<float>> qs((size_t)n, std::vector<float>((size_t)dim));
    for (int i = 0; i < n; ++i) {
        double s = 0;
        auto& q = qs[(size_t)i];
        // every fourth query is concentrated on a few coordinates, or all of one sign
        // (the largest |q|_1 and sum q the bias term sees)
        for (int j = 0; j < dim; ++j) {
            float v = nd(rng);
            if (i % 4 == 1) v = j % 97 == i % 97 ? v * 30.f : v * 0.01f;
            if (i % 4 == 2) v = std::fabs(v);
            q[(size_t)j] = v;
            s += (double)v * v;
        }
        const double inv = 1.0 / std::sqrt(s);
        for (int j = 0; j < dim; ++j) q[(size_t)j] = (float)(q[(size_t)j] * inv);
    }
    return qs;
}

// the kernels' arithmetic: f32 FMA sums (sequential here; the bound holds for any order)
static float f32_dot(const float* a, const float* b, int n) {
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc = std::fmaf(a[i], b[i], acc);
    return acc;
}

static void check_row(const char* what, const std::vector<float>& x, const std::vector<std::vector<float>>& qs,
                      bool expect_inf) {
    const int dim = (int)x.size();
    std::vector<uint8_t> u(vsg::sketch_stride(dim) + 1, 0xAB);
    const SketchMeta m = vsg::sketch_row(x.data(), dim, u.data());
    CHECK(u[vsg::sketch_stride(dim)] == 0xAB, "%s: wrote past the sketch row", what);
    for (size_t i = (size_t)dim; i < vsg::sketch_stride(dim); ++i) CHECK(u[i] == 128, "%s: padding byte %zu", what, i);
    if (expect_inf) {
        CHECK(std::isinf(m.err) && m.err > 0, "%s: err = %g, expected +inf", what, (double)m.err);
        CHECK(m.scale == 0.f, "%s: scale = %g of an unusable row", what, (double)m.scale);
        return;
    }
    CHECK(std::isfinite(m.err) && m.err >= 0 && m.scale > 0, "%s: err %g scale %g", what, (double)m.err, (double)m.scale);
    if (!std::isfinite(m.err)) return;
    // |x - x~| itself
    double r2 = 0;
    for (int i = 0; i < dim; ++i) {
        const double xt = (double)m.scale * ((int)u[(size_t)i] - 128);
        r2 += ((double)x[(size_t)i] - xt) * ((double)x[(size_t)i] - xt);
    }
    CHECK(std::sqrt(r2) <= (double)m.err, "%s: |x - x~| = %g > err = %g", what, std::sqrt(r2), (double)m.err);
    std::vector<float> uf((size_t)dim);
    for (int i = 0; i < dim; ++i) uf[(size_t)i] = (float)u[(size_t)i];
    for (const auto& q : qs) {
        double dx = 0, dxt = 0, q2 = 0;
        for (int i = 0; i < dim; ++i) {
            dx += (double)q[(size_t)i] * x[(size_t)i];
            dxt += (double)q[(size_t)i] * ((double)m.scale * ((int)u[(size_t)i] - 128));
            q2 += (double)q[(size_t)i] * q[(size_t)i];
        }
        const double qn = std::sqrt(q2);
        CHECK(std::fabs(dx - dxt) <= (double)m.err * qn, "%s: |q.x - q.x~| = %g > |q| err = %g", what,
              std::fabs(dx - dxt), (double)m.err * qn);
        // the search's own f32 arithmetic: bound and exact distance
        float sumq = 0.f, sq2 = 0.f;
        for (int i = 0; i < dim; ++i) {
            sumq += q[(size_t)i];
            sq2 = std::fmaf(q[(size_t)i], q[(size_t)i], sq2);
        }
        const float qup = vsg::sketch_qnorm_up(sq2, dim);
        CHECK((double)qup >= qn, "%s: |q| bound %g < %g", what, (double)qup, qn);
        const float t = f32_dot(uf.data(), q.data(), dim) - 128.f * sumq;
        const float ub = std::fmaf(qup, m.err, m.scale * t);
        const float lower = 1.f - ub;
        const float exact = 1.f - f32_dot(x.data(), q.data(), dim);
        CHECK(lower <= exact, "%s: bound %.9g > f32 distance %.9g", what, (double)lower, (double)exact);
        CHECK((double)ub >= dx, "%s: f32 upper bound %.9g < q.x = %.9g", what, (double)ub, dx);
    }
}

int main() {
    const int dims[] = {768, 1536, 264, 5};
    const int NQ = 1000;
    std::mt19937_64 rng(12345);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::cauchy_distribution<float> cd(0.f, 1.f);
    const float inf = std::numeric_limits<float>::infinity();
    for (int dim : dims) {
        const auto qs = unit_queries(dim, NQ, 777u + (uint64_t)dim);
        std::vector<float> x((size_t)dim);
        auto normalise = [&]() {
            double s = 0;
            for (float v : x) s += (double)v * v;
            for (float& v : x) v = (float)(v / std::sqrt(s));
        };
        // random unit rows, and the same rows at other norms
        for (int rep = 0; rep < 3; ++rep) {
            for (float& v : x) v = nd(rng);
            normalise();
            check_row("random unit", x, qs, false);
            for (float& v : x) v *= 37.5f;
            check_row("random x37.5", x, qs, false);
            for (float& v : x) v *= 1e-6f;
            check_row("random small", x, qs, false);
        }
        // heavy-tailed: Cauchy elements, and one 1e6 outlier among unit-scale ones
        for (int rep = 0; rep < 3; ++rep) {
            for (float& v : x) v = cd(rng);
            check_row("cauchy", x, qs, false);
            normalise();
            check_row("cauchy unit", x, qs, false);
        }
        for (float& v : x) v = nd(rng);
        x[(size_t)dim / 2] = 1e6f;
        check_row("outlier 1e6", x, qs, false);
        // one-hot and constant rows
        for (float& v : x) v = 0.f;
        x[1] = 1.f;
        check_row("one-hot", x, qs, false);
        for (float& v : x) v = 0.25f;
        check_row("constant", x, qs, false);
        // denormal rows: no usable scale -> never rejected
        for (float& v : x) v = nd(rng) * 1e-41f;
        check_row("denormal", x, qs, true);
        for (float& v : x) v = nd(rng) * 1e-36f;  // normal but tiny: still bounded or +inf, never wrong
        {
            std::vector<uint8_t> u(vsg::sketch_stride(dim));
            const SketchMeta m = vsg::sketch_row(x.data(), dim, u.data());
            check_row("tiny", x, qs, std::isinf(m.err));
        }
        // all-zero
        for (float& v : x) v = 0.f;
        check_row("all-zero", x, qs, true);
        // non-finite
        for (float& v : x) v = nd(rng);
        x[0] = inf;
        check_row("+inf element", x, qs, true);
        x[0] = -inf;
        check_row("-inf element", x, qs, true);
        x[0] = std::numeric_limits<float>::quiet_NaN();
        check_row("NaN element", x, qs, true);
        x[0] = 1.f;
        x[(size_t)dim - 1] = std::numeric_limits<float>::quiet_NaN();
        check_row("NaN last", x, qs, true);
        // huge: the scale would overflow the slack terms
        for (float& v : x) v = nd(rng) * 1e35f;
        check_row("huge", x, qs, true);
    }
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

// The integer sketch pass of csrc/sketch.hpp on the CPU: the query's 16-bit quantisation in
// two int8 planes (sketch_qscale / sketch_q16 / _hi / _lo / sketch_query) and the kernel's f32
// bound (sketch_upper), the functions the device code calls, for dims 256, 264, 768, 1536,
// 2048 (above 1040 the int -> f32 conversions of the sums are inexact), the row families of
// test_sketch_bound.cpp and random-unit, one-hot, constant +-max, heavy-tailed, 1e20 / 1e-20
// scaled and un-normalised queries:
//   the planes reconstruct q16 exactly and lie in [-127, 127] / [-128, 127];
//   H and L (int32, as v_dot4 accumulates them) equal an int64 recomputation;
//   the f32 upper bound is >= q.x in f64 plus the f32 exact pass's worst rounding
//   g_d sum |q_i x_i| (any summation order), and 1 - bound <= the sequential f32 distance;
//   all-zero, non-finite and out-of-range queries report "no filter" (sq == 0).
// Stand-alone: g++ -fsanitize=address,undefined tests/cpp/test_sketch_bound_i8.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../vector-store-text_amd/csrc/sketch.hpp"

using vsg::SketchMeta;
using vsg::SketchQuery;

static int g_fail = 0;
static long g_usable = 0, g_bounds = 0;
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

// What SketchQ::stage computes for one query: planes and the three numbers.
struct QImage {
    std::vector<int8_t> h, l;
    SketchQuery k;
};

static QImage stage(const char* what, const std::vector<float>& q, size_t stride) {
    const int dim = (int)q.size();
    QImage im;
    im.h.assign(stride, 0);
    im.l.assign(stride, 0);
    const float mx = vsg::sketch_maxabs(q.data(), dim);
    float s2 = 0.f;
    for (int i = 0; i < dim; ++i) s2 = std::fmaf(q[(size_t)i], q[(size_t)i], s2);
    const float sq = vsg::sketch_qscale(mx);
    float r2 = 0.f;
    double r2d = 0;
    if (sq > 0.f) {
        for (int i = 0; i < dim; ++i) {
            const int q16 = vsg::sketch_q16(q[(size_t)i], sq);
            const int h = vsg::sketch_q16_hi(q16), l = vsg::sketch_q16_lo(q16);
            CHECK(q16 >= -32512 && q16 <= 32512, "%s: q16 %d", what, q16);
            CHECK(h >= -127 && h <= 127 && l >= -128 && l <= 127, "%s: planes %d %d of %d", what, h, l, q16);
            CHECK(256 * h + l == q16, "%s: planes %d %d do not give %d", what, h, l, q16);
            im.h[(size_t)i] = (int8_t)h;
            im.l[(size_t)i] = (int8_t)l;
            r2 += vsg::sketch_qres2(q[(size_t)i], sq, q16);
            const double r = (double)q[(size_t)i] - (double)sq * q16;
            r2d += r * r;
        }
    }
    im.k = vsg::sketch_query(mx, r2, s2, dim);
    if (im.k.sq > 0.f) {
        double n2 = 0;
        for (float v : q) n2 += (double)v * v;
        CHECK((double)im.k.qn >= std::sqrt(n2), "%s: |q| bound %g < %g", what, (double)im.k.qn, std::sqrt(n2));
        // qe = qerr 127 sqrt(d) rounded up
        CHECK((double)im.k.qe >= std::sqrt(r2d) * 127.0 * std::sqrt((double)dim), "%s: qe %g < %g", what,
              (double)im.k.qe, std::sqrt(r2d) * 127.0 * std::sqrt((double)dim));
    }
    return im;
}

struct Row {
    const char* what;
    std::vector<float> x;
    std::vector<uint8_t> u;
    SketchMeta m;
};

static void check_pair(const Row& r, const char* qwhat, const std::vector<float>& q, const QImage& im) {
    const int dim = (int)q.size();
    if (!(im.k.sq > 0.f)) return;
    ++g_usable;
    // the integer sums as the kernel forms them (int32 accumulators), against int64
    int32_t H = 0, L = 0;
    int64_t H64 = 0, L64 = 0;
    for (size_t i = 0; i < r.u.size(); ++i) {
        const int xs = (int)(int8_t)(r.u[i] ^ 0x80);
        CHECK(xs == (int)r.u[i] - 128, "%s: signed byte %d of %d", r.what, xs, (int)r.u[i]);
        H += xs * im.h[i];
        L += xs * im.l[i];
        H64 += (int64_t)xs * im.h[i];
        L64 += (int64_t)xs * im.l[i];
    }
    CHECK(H == H64 && L == L64, "%s / %s: int32 sums %d %d != %lld %lld", r.what, qwhat, H, L, (long long)H64,
          (long long)L64);
    const float ub = vsg::sketch_upper(im.k, r.m, H, L);
    if (!(std::fabs(ub) < std::numeric_limits<float>::infinity())) return;  // the kernel keeps the candidate
    ++g_bounds;
    double dx = 0, ax = 0;
    float f32 = 0.f;
    for (int i = 0; i < dim; ++i) {
        dx += (double)q[(size_t)i] * r.x[(size_t)i];
        ax += std::fabs((double)q[(size_t)i] * r.x[(size_t)i]);
        f32 = std::fmaf(r.x[(size_t)i], q[(size_t)i], f32);
    }
    const double u = std::ldexp(1.0, -24), gd = dim * u / (1.0 - dim * u);
    CHECK((double)ub >= dx + gd * ax, "%s / %s (d %d): f32 upper bound %.9g < q.x + g_d sum|q x| = %.9g", r.what, qwhat,
          dim, (double)ub, dx + gd * ax);
    CHECK(1.f - ub <= 1.f - f32, "%s / %s (d %d): bound %.9g > f32 distance %.9g", r.what, qwhat, dim,
          (double)(1.f - ub), (double)(1.f - f32));
}

int main() {
    const int dims[] = {256, 264, 768, 1536, 2048};
    const int NQ = 200;
    std::mt19937_64 rng(4242);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::cauchy_distribution<float> cd(0.f, 1.f);
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int dim : dims) {
        const size_t stride = vsg::sketch_stride(dim);
        auto unit = [](std::vector<float>& v) {
            double s = 0;
            for (float e : v) s += (double)e * e;
            for (float& e : v) e = (float)(e / std::sqrt(s));
        };
        // ---- rows: the families of test_sketch_bound.cpp
        std::vector<Row> rows;
        auto add_row = [&](const char* what, const std::vector<float>& x, int expect_inf) {
            Row r{what, x, std::vector<uint8_t>(stride), {}};
            r.m = vsg::sketch_row(x.data(), dim, r.u.data());
            if (expect_inf >= 0) CHECK((std::isinf(r.m.err) != 0) == (expect_inf != 0), "%s: err %g", what, (double)r.m.err);
            rows.push_back(r);
        };
        std::vector<float> x((size_t)dim);
        for (int rep = 0; rep < 2; ++rep) {
            for (float& v : x) v = nd(rng);
            unit(x);
            add_row("random unit", x, 0);
            for (float& v : x) v *= 37.5f;
            add_row("random x37.5", x, 0);
            for (float& v : x) v *= 1e-6f;
            add_row("random small", x, 0);
            for (float& v : x) v = cd(rng);
            add_row("cauchy", x, 0);
            unit(x);
            add_row("cauchy unit", x, 0);
        }
        for (float& v : x) v = nd(rng);
        x[(size_t)dim / 2] = 1e6f;
        add_row("outlier 1e6", x, 0);
        for (float& v : x) v = 0.f;
        x[1] = 1.f;
        add_row("one-hot", x, 0);
        for (float& v : x) v = 0.25f;
        add_row("constant", x, 0);
        for (float& v : x) v = -3.f;
        add_row("constant negative", x, 0);
        for (float& v : x) v = nd(rng) * 1e-41f;
        add_row("denormal", x, 1);
        for (float& v : x) v = nd(rng) * 1e-29f;
        add_row("tiny", x, -1);
        for (float& v : x) v = nd(rng) * 1e29f;
        add_row("large", x, -1);
        for (float& v : x) v = 0.f;
        add_row("all-zero", x, 1);
        for (float& v : x) v = nd(rng);
        x[0] = inf;
        add_row("+inf element", x, 1);
        x[0] = nan;
        add_row("NaN element", x, 1);
        for (float& v : x) v = nd(rng) * 1e35f;
        add_row("huge", x, 1);

        // ---- queries
        struct Q {
            const char* what;
            std::vector<float> q;
            int usable;  // 1 yes, 0 no, -1 either
        };
        std::vector<Q> qs;
        std::vector<float> q((size_t)dim);
        for (int i = 0; i < NQ; ++i) {
            for (int j = 0; j < dim; ++j) {
                float v = nd(rng);
                if (i % 4 == 1) v = j % 97 == i % 97 ? v * 30.f : v * 0.01f;
                if (i % 4 == 2) v = std::fabs(v);
                q[(size_t)j] = v;
            }
            unit(q);
            qs.push_back({"random unit", q, 1});
        }
        for (int i = 0; i < 20; ++i) {
            for (float& v : q) v = cd(rng);
            qs.push_back({"heavy-tailed", q, -1});
            unit(q);
            qs.push_back({"heavy-tailed unit", q, 1});
            for (float& v : q) v = nd(rng) * (0.01f + 50.f * (float)i);
            qs.push_back({"un-normalised", q, 1});
            for (float& v : q) v = nd(rng);
            unit(q);
            for (float& v : q) v *= 1e20f;
            qs.push_back({"scaled 1e20", q, 0});
            for (float& v : q) v *= 1e-20f * 1e-20f;
            qs.push_back({"scaled 1e-20", q, 0});
        }
        for (int hot : {0, 1, dim - 1}) {
            for (float& v : q) v = 0.f;
            q[(size_t)hot] = hot == 1 ? -1.f : 1.f;
            qs.push_back({"one-hot", q, 1});
        }
        // constant +-max: every h and l at the ends of their ranges
        for (float& v : q) v = 0.0361f;
        qs.push_back({"constant +max", q, 1});
        for (float& v : q) v = -0.0361f;
        qs.push_back({"constant -max", q, 1});
        for (int j = 0; j < dim; ++j) q[(size_t)j] = (j & 1) ? 7.5f : -7.5f;
        qs.push_back({"alternating +-max", q, 1});
        // q16 = +-128 / +-127 / 32511: the planes' carries
        for (int j = 0; j < dim; ++j) {
            const int k16[] = {128, -128, 127, -129, 32511, -32511, 255, -256};
            q[(size_t)j] = (float)k16[j % 8] / 32512.f;
        }
        q[0] = 1.f;
        qs.push_back({"plane carries", q, 1});
        // the ends of the usable range
        for (float& v : q) v = nd(rng);
        unit(q);
        for (float& v : q) v *= 1e-10f;
        qs.push_back({"scaled 1e-10", q, 1});
        for (float& v : q) v *= 1e20f;
        qs.push_back({"scaled 1e10", q, 1});
        // unusable
        for (float& v : q) v = 0.f;
        qs.push_back({"all-zero", q, 0});
        for (float& v : q) v = nd(rng);
        q[3] = inf;
        qs.push_back({"+inf element", q, 0});
        q[3] = -inf;
        qs.push_back({"-inf element", q, 0});
        q[3] = 1.f;
        q[(size_t)dim - 1] = nan;
        qs.push_back({"NaN last", q, 0});
        for (float& v : q) v = 1e-42f;
        qs.push_back({"denormal", q, 0});
        for (float& v : q) v = 3e38f;
        qs.push_back({"near overflow", q, 0});

        for (const Q& e : qs) {
            const QImage im = stage(e.what, e.q, stride);
            if (e.usable == 1) CHECK(im.k.sq > 0.f, "%s (d %d): no filter for a usable query", e.what, dim);
            if (e.usable == 0) CHECK(im.k.sq == 0.f, "%s (d %d): sq = %g, expected no filter", e.what, dim, (double)im.k.sq);
            for (const Row& r : rows) check_pair(r, e.what, e.q, im);
        }
    }
    CHECK(g_bounds > 10000, "only %ld finite bounds checked", g_bounds);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("%ld usable (query, row) pairs, %ld finite bounds\nok\n", g_usable, g_bounds);
    return 0;
}

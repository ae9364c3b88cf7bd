// misc.hip — row preparation (f32 -> storage type, cos normalisation),
// tombstone scatter and the HBM synthetic-data generator.
//
// Every kernel here walks its rows / elements with a grid-stride loop over a
// capped grid: the AQL dispatch packet counts work-items in 32 bits, so a
// one-wave-per-row launch overflows beyond 2^32 / 64 = 67M rows (C4 is 100M).
#include <hip/hip_runtime.h>

#include "sketch.hpp"
#include "vsg_device.hpp"
#include "vsg_kernels.hpp"

namespace vsg {

// blocks for `items` work units of `per_block` each, capped well below the 2^32
// work-item limit of one dispatch (kernels loop over the remainder)
static inline unsigned capped_grid(size_t items, size_t per_block, size_t cap = 1u << 20) {
    size_t g = (items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (unsigned)(g < cap ? g : cap);
}

// One wave per row.  Cos rows are stored unit-normalised (x / |x|) so the
// traversal kernels evaluate cos as 1 - dot.
template <typename T>
__global__ __launch_bounds__(256) void prepare_kernel(const float* __restrict__ in, size_t n, int dim,
                                                      int normalize, uint8_t* __restrict__ out,
                                                      size_t row_bytes, float* __restrict__ sqnorm) {
    const int lane = threadIdx.x & 63;
    const int padded = (int)(row_bytes / sizeof(T));
    for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (size_t)gridDim.x * 4) {
        const float* x = in + row * (size_t)dim;
        T* y = reinterpret_cast<T*>(out + row * row_bytes);
        float nrm = 1.f;
        if (normalize) {
            float s = 0.f;
            for (int j = lane; j < dim; j += 64) s += x[j] * x[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            nrm = sqrtf(s);
        }
        float s2 = 0.f;
        for (int j = lane; j < padded; j += 64) {
            float v = 0.f;
            if (j < dim) v = (normalize && nrm > 0.f) ? x[j] / nrm : (normalize ? 0.f : x[j]);
            const T t = (T)v;
            y[j] = t;
            s2 += (float)t * (float)t;
        }
        if (sqnorm) {  // |stored row|^2 for the MFMA L2 expansion |x|^2 + |q|^2 - 2 x.q
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
            if (lane == 0) sqnorm[row] = s2;
        }
    }
}

template <typename T>
__global__ void unprepare_kernel(const uint8_t* __restrict__ in, size_t n, int dim, size_t row_bytes,
                                 float* __restrict__ out) {
    const size_t tot = n * (size_t)dim;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / dim;
        const int j = (int)(i % dim);
        out[i] = (float)reinterpret_cast<const T*>(in + r * row_bytes)[j];
    }
}

hipError_t launch_prepare(Storage st, const float* in, size_t n, int dim, bool normalize, uint8_t* out,
                          size_t row_bytes, hipStream_t s, float* sqnorm) {
    if (n == 0) return hipSuccess;
    const dim3 grid(capped_grid(n, 4));
    if (st == ST_F32)
        hipLaunchKernelGGL(prepare_kernel<float>, grid, dim3(256), 0, s, in, n, dim, normalize ? 1 : 0, out, row_bytes,
                           sqnorm);
    else
        hipLaunchKernelGGL(prepare_kernel<_Float16>, grid, dim3(256), 0, s, in, n, dim, normalize ? 1 : 0, out,
                           row_bytes, sqnorm);
    return hipGetLastError();
}

hipError_t launch_unprepare(Storage st, const uint8_t* in, size_t n, int dim, size_t row_bytes, float* out,
                            hipStream_t s) {
    const size_t tot = n * (size_t)dim;
    if (tot == 0) return hipSuccess;
    const dim3 grid(capped_grid(tot, 256));
    if (st == ST_F32)
        hipLaunchKernelGGL(unprepare_kernel<float>, grid, dim3(256), 0, s, in, n, dim, row_bytes, out);
    else
        hipLaunchKernelGGL(unprepare_kernel<_Float16>, grid, dim3(256), 0, s, in, n, dim, row_bytes, out);
    return hipGetLastError();
}

__global__ void set_flags_kernel(uint8_t* flags, const uint32_t* slots, size_t n, uint8_t value) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        flags[slots[i]] = value;
}

hipError_t launch_set_flags(uint8_t* flags, const uint32_t* slots, size_t n, uint8_t value, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(set_flags_kernel, dim3(capped_grid(n, 256)), dim3(256), 0, s, flags, slots, n, value);
    return hipGetLastError();
}

// Compaction gather (vsg_index_compact): live slot idx[i] -> row i of the new
// image.  One wave per row, 16-B vector loads/stores (rows are 16-B multiples).
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint8_t* __restrict__ vecs,
                                                          const float* __restrict__ sqnorm,
                                                          const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ idx, size_t n,
                                                          size_t row_bytes, uint8_t* __restrict__ out_vecs,
                                                          float* __restrict__ out_sq, uint64_t* __restrict__ out_keys) {
    const int lane = threadIdx.x & 63;
    const size_t n16 = row_bytes / 16;
    for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (size_t)gridDim.x * 4) {
        const size_t src = idx[row];
        const uint4* a = reinterpret_cast<const uint4*>(vecs + src * row_bytes);
        uint4* b = reinterpret_cast<uint4*>(out_vecs + row * row_bytes);
        for (size_t c = lane; c < n16; c += 64) b[c] = a[c];
        if (lane == 0) {
            out_sq[row] = sqnorm[src];
            out_keys[row] = keys[src];
        }
    }
}

hipError_t launch_gather_rows(const uint8_t* vecs, const float* sqnorm, const uint64_t* keys, const uint32_t* idx,
                              size_t n, size_t row_bytes, uint8_t* out_vecs, float* out_sq, uint64_t* out_keys,
                              hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(capped_grid(n, 4)), dim3(256), 0, s, vecs, sqnorm, keys, idx, n,
                       row_bytes, out_vecs, out_sq, out_keys);
    return hipGetLastError();
}

// ------------------------------------------------------- locality cells --
// Build scheduling only (vsg_index.cpp build_slots): nearest pivot of each row
// from the MFMA exact search's partial lists, and per-batch sort keys.

__global__ void nearest_part_kernel(const float* __restrict__ part_d, const uint32_t* __restrict__ part_i, int nq,
                                    int parts, int kin, uint32_t* __restrict__ out) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nq; r += gridDim.x * blockDim.x) {
        float bd = __builtin_inff();
        uint32_t bi = 0;
        const size_t base = (size_t)r * parts * kin;
        for (int j = 0; j < parts * kin; ++j) {
            const uint32_t id = part_i[base + j];
            const float d = part_d[base + j];
            if (id != 0xFFFFFFFFu && d < bd) {
                bd = d;
                bi = id;
            }
        }
        out[r] = bi;
    }
}

hipError_t launch_nearest_part(const float* part_d, const uint32_t* part_i, int nq, int parts, int kin,
                               uint32_t* out, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(nearest_part_kernel, dim3(capped_grid((size_t)nq, 256)), dim3(256), 0, s, part_d, part_i, nq,
                       parts, kin, out);
    return hipGetLastError();
}

__global__ void batch_keys_kernel(const uint32_t* __restrict__ nodes, int n, uint32_t s0,
                                  const uint32_t* __restrict__ cell, uint64_t* __restrict__ okey,
                                  uint32_t* __restrict__ oidx) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
        okey[b] = ((uint64_t)cell[nodes[b] - s0] << 32) | (uint32_t)b;
        oidx[b] = (uint32_t)b;
    }
}

hipError_t launch_batch_keys(const uint32_t* nodes, int n, uint32_t s0, const uint32_t* cell, uint64_t* okey,
                             uint32_t* oidx, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(batch_keys_kernel, dim3(capped_grid((size_t)n, 256)), dim3(256), 0, s, nodes, n, s0, cell,
                       okey, oidx);
    return hipGetLastError();
}

// ---------------------------------------------------------------- datagen --
// Same formulas and stream tags as vector-store-text_amd/vsg/datagen.py.

__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr uint64_t TAG_CLUSTER = 0x436C7573, TAG_LATENT = 0x4C6174, TAG_NOISE = 0x4E6F6973,
                   TAG_CENTRE = 0x43656E74, TAG_PROJ = 0x50726F6A, TAG_U8 = 0x55380000;
constexpr int N_CENTRES = 1024, LATENT = 64;

__device__ inline double uniform01(uint64_t base, uint64_t idx) {
    const uint64_t r = splitmix64(base + idx);
    return ((double)(r >> 11) + 1.0) * (1.0 / 9007199254740992.0);
}

__device__ inline float normal_at(uint64_t base, uint64_t idx) {
    const double u1 = uniform01(base, 2 * idx);
    const double u2 = uniform01(base, 2 * idx + 1);
    return (float)(sqrt(-2.0 * log(u1)) * cos(2.0 * 3.141592653589793 * u2));
}

__global__ void gen_normal_kernel(uint64_t base, size_t count, float scale, float* out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        out[i] = normal_at(base, i) / scale;
}

// kind 0 (clustered) / 3 (SIFT-like: ReLU, x48, rounded into 0..255); one wave per row
__global__ __launch_bounds__(64) void gen_clustered_kernel(size_t n, int dim, uint64_t seed, size_t start,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ centres, int sift,
                                                           float* __restrict__ out) {
    __shared__ float lat[LATENT];
    const int lane = threadIdx.x;
    const uint64_t cbase = splitmix64(seed ^ TAG_CLUSTER);
    const uint64_t lbase = splitmix64(seed ^ TAG_LATENT);
    const uint64_t nbase = splitmix64(seed ^ TAG_NOISE);
    for (size_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint64_t row = start + r;
        const uint64_t cl = splitmix64(cbase + row) % N_CENTRES;
        __syncthreads();  // previous row's readers are done with lat[]
        lat[lane] = centres[cl * LATENT + lane] + 0.5f * normal_at(lbase, row * LATENT + lane);
        __syncthreads();
        for (int j = lane; j < dim; j += 64) {
            float acc = 0.f;
            for (int l = 0; l < LATENT; ++l) acc += lat[l] * w[(size_t)l * dim + j];
            float v = acc + 0.05f * normal_at(nbase, row * (uint64_t)dim + j);
            if (sift) v = fminf(255.f, rintf(fmaxf(v, 0.f) * 48.f));
            out[r * dim + j] = v;
        }
    }
}

__global__ void gen_gauss_kernel(size_t n, int dim, uint64_t seed, size_t start, float* out) {
    const size_t tot = n * (size_t)dim;
    const uint64_t nbase = splitmix64(seed ^ TAG_NOISE);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x)
        out[i] = normal_at(nbase, start * (uint64_t)dim + i);
}

__global__ void gen_u8_kernel(size_t n, int dim, uint64_t seed, size_t start, float* out) {
    const size_t tot = n * (size_t)dim;
    const uint64_t b = splitmix64(seed ^ TAG_U8);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x)
        out[i] = (float)(splitmix64(b + start * (uint64_t)dim + i) % 256);
}

hipError_t launch_datagen(int kind, size_t n, size_t dim, uint64_t seed, uint64_t model_seed, size_t start_row,
                          float* out, float* scratch_w, float* scratch_c, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const size_t tot = n * dim;
    if (kind == 0 || kind == 3) {
        const size_t nw = (size_t)LATENT * dim, ncen = (size_t)N_CENTRES * LATENT;
        hipLaunchKernelGGL(gen_normal_kernel, dim3(capped_grid(nw, 256)), dim3(256), 0, s,
                           splitmix64(model_seed ^ TAG_PROJ), nw, 8.0f, scratch_w);
        hipLaunchKernelGGL(gen_normal_kernel, dim3(capped_grid(ncen, 256)), dim3(256), 0, s,
                           splitmix64(model_seed ^ TAG_CENTRE), ncen, 1.0f, scratch_c);
        hipLaunchKernelGGL(gen_clustered_kernel, dim3(capped_grid(n, 1)), dim3(64), 0, s, n, (int)dim, seed,
                           start_row, scratch_w, scratch_c, kind == 3 ? 1 : 0, out);
    } else if (kind == 1) {
        hipLaunchKernelGGL(gen_gauss_kernel, dim3(capped_grid(tot, 256)), dim3(256), 0, s, n, (int)dim, seed,
                           start_row, out);
    } else {
        hipLaunchKernelGGL(gen_u8_kernel, dim3(capped_grid(tot, 256)), dim3(256), 0, s, n, (int)dim, seed,
                           start_row, out);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------ int8 sketch --
// f32 rows [r0, r1) -> sketch rows (sketch.hpp: bytes, and (scale, err) in meta).
// One wave per row, one 4-element group per lane and step; the reductions are
// wave-wide, the values those of sketch_row().
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void sketch_rows_kernel(const uint8_t* __restrict__ vecs, size_t row_bytes, size_t r0,
                                                          size_t r1, int dim, uint8_t* __restrict__ out, size_t stride,
                                                          SketchMeta* __restrict__ meta) {
    const int lane = threadIdx.x & 63;
    const int ngroups = (dim + 3) / 4;          // 4-element groups holding the row (row_bytes >= 4 * dim rounded to 16)
    const int sgroups = (int)(stride / 4);      // groups of the sketch row (>= ngroups)
    for (size_t row = r0 + (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < r1; row += (size_t)gridDim.x * 4) {
        const float4* src = reinterpret_cast<const float4*>(vecs + row * row_bytes);
        uint32_t* dst = reinterpret_cast<uint32_t*>(out + row * stride);
        bool bad = false;
        float mx = 0.f;
        for (int g = lane; g < ngroups; g += 64) {
            const float4 v = src[g];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (g * 4 + j < dim) {
                    const float a = fabsf(e[j]);
                    bad = bad || !(a <= 3.4028234e38f);
                    mx = fmaxf(mx, a);
                }
            }
        }
        mx = wave_max_f32(mx);
        const bool anybad = __ballot(bad) != 0;
        const float scale = anybad ? 0.f : sketch_scale(mx);
        float r2 = 0.f, x2 = 0.f;
        for (int g = lane; g < sgroups; g += 64) {
            uint32_t w = 0x80808080u;
            if (scale > 0.f && g < ngroups) {
                const float4 v = src[g];
                const float e[4] = {v.x, v.y, v.z, v.w};
                w = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint8_t u = 128;
                    if (g * 4 + j < dim) {
                        u = sketch_quant(e[j], scale);
                        r2 += sketch_res2(e[j], scale, u);
                        x2 = fmaf(e[j], e[j], x2);
                    }
                    w |= (uint32_t)u << (8 * j);
                }
            }
            dst[g] = w;
        }
        r2 = wave_sum_f32(r2);
        x2 = wave_sum_f32(x2);
        if (lane == 0) {
            SketchMeta m;
            m.err = sketch_err(r2, x2, scale, dim);
            m.scale = m.err < INFINITY ? scale : 0.f;
            meta[row] = m;
        }
    }
}

hipError_t launch_sketch_rows(const uint8_t* vecs, size_t row_bytes, size_t r0, size_t r1, int dim, uint8_t* out,
                              void* meta, hipStream_t s) {
    if (r1 <= r0) return hipSuccess;
    hipLaunchKernelGGL(sketch_rows_kernel, dim3(capped_grid(r1 - r0, 4)), dim3(256), 0, s, vecs, row_bytes, r0, r1, dim,
                       out, sketch_stride(dim), reinterpret_cast<SketchMeta*>(meta));
    return hipGetLastError();
}

}  // namespace vsg

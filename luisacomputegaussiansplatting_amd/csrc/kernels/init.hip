// init.hip -- a scene from a point cloud: 3DGS's create_from_pcd.  Every splat's initial scale comes from the
// mean squared distance to its three nearest neighbours, an EXACT k-nearest-neighbour query over the whole cloud; the
// definition (include/lcgs_hip.h) fixes every binary32 operation, so the result is a pure function of the multiset of points.
//   1. box      exact min / max and count of the finite points: per-block partials, one finishing block (no atomics).  The box
//               only shapes the Morton grid; no result depends on it.
//   2. sort     30-bit Morton keys (ingest.hip) through the stable pair sort (pair_sort.hip); non-finite points land in cell 0
//   3. gather   sorted[r] = (x, y, z, bits(original index)) and, per chunk of kKnnChunk sorted points, the box of its finite points
//   4. query    one workgroup per chunk, one query per lane, the three smallest d2 in registers: the own chunk from LDS, then
//               the other chunks outward along the curve -- whole chunks skipped by a box-to-box bound against the workgroup's
//               largest third-best, lanes sitting out by their own point-to-box bound
//   5. rows     the five parameter arrays in the CALLER's order (the sort leaves no trace in the outputs)
#include <math.h>

#include "activations.hpp"
#include "launch.hpp"

namespace lcgs
{
namespace
{

constexpr int kBoxBlocks = 256;
struct BoxPartial {
    float    lo[3], hi[3];
    uint32_t count, pad;
};

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; // (NaN compares false)
}

// min / max of six values and a count over the workgroup's 256 threads -> thread 0 holds the result
__device__ __forceinline__ void block_box(float lo[3], float hi[3], uint32_t& count)
{
    __shared__ float    s_box[4][6];
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
        }
        if (lane == 0) {
            s_box[wave][a]     = lo[a];
            s_box[wave][3 + a] = hi[a];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
    if (lane == 0) s_cnt[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(fminf(s_box[0][a], s_box[1][a]), fminf(s_box[2][a], s_box[3][a]));
            hi[a] = fmaxf(fmaxf(s_box[0][3 + a], s_box[1][3 + a]), fmaxf(s_box[2][3 + a], s_box[3][3 + a]));
        }
        count = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}

__global__ void __launch_bounds__(256) k_knn_box_partial(int64_t n, const float* __restrict__ pos, BoxPartial* __restrict__ partial)
{
    float    lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    uint32_t count = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float p[3] = { pos[3 * i], pos[3 * i + 1], pos[3 * i + 2] };
        if (!finite3(p[0], p[1], p[2])) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], p[a]);
            hi[a] = fmaxf(hi[a], p[a]);
        }
        ++count;
    }
    block_box(lo, hi, count);
    if (threadIdx.x == 0) {
        BoxPartial b;
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = lo[a];
            b.hi[a] = hi[a];
        }
        b.count = count;
        b.pad   = 0;
        partial[blockIdx.x] = b;
    }
}

__global__ void __launch_bounds__(256) k_knn_box_finish(int blocks, const BoxPartial* __restrict__ partial, KnnGrid* __restrict__ grid)
{
    float    lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    uint32_t count = 0;
    if ((int)threadIdx.x < blocks) {
        const BoxPartial b = partial[threadIdx.x];
        for (int a = 0; a < 3; ++a) {
            lo[a] = b.lo[a];
            hi[a] = b.hi[a];
        }
        count = b.count;
    }
    block_box(lo, hi, count);
    if (threadIdx.x == 0) {
        KnnGrid g;
        for (int a = 0; a < 3; ++a) {
            // 1024 cells over the box; a flat axis (or no finite point at all) gets one cell.  Locality only.
            const float extent = hi[a] - lo[a];
            const bool  usable = count > 0 && extent > 0.0f && extent < INFINITY;
            g.lo[a]            = count > 0 ? lo[a] : 0.0f;
            g.cells[a]         = usable ? 1024.0f / extent : 0.0f;
        }
        g.num_valid = count;
        g.pad       = 0;
        *grid       = g;
    }
}

__global__ void __launch_bounds__(kKnnChunk) k_knn_gather_boxes(int64_t n, const float* __restrict__ pos,
                                                                const uint32_t* __restrict__ perm, float4* __restrict__ sorted,
                                                                float4* __restrict__ boxes)
{
    const int64_t r     = (int64_t)blockIdx.x * kKnnChunk + threadIdx.x;
    float         lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    uint32_t      count = 0;
    if (r < n) {
        const uint32_t i    = perm[r];
        const float    p[3] = { pos[3 * (int64_t)i], pos[3 * (int64_t)i + 1], pos[3 * (int64_t)i + 2] };
        sorted[r]           = make_float4(p[0], p[1], p[2], __uint_as_float(i));
        if (finite3(p[0], p[1], p[2])) {
            for (int a = 0; a < 3; ++a) lo[a] = hi[a] = p[a];
            count = 1;
        }
    }
    block_box(lo, hi, count);
    if (threadIdx.x == 0) {
        boxes[2 * (int64_t)blockIdx.x]     = make_float4(lo[0], lo[1], lo[2], 0.0f);
        boxes[2 * (int64_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The query.  d2 is the contract's expression, written once; the two lower bounds use THE SAME operations in the same order
// on per-axis gaps, which is what makes the pruning exact in floating point and not only in real arithmetic:
//   for p inside a box and a query q left of it, p - q >= lo - q exactly, and round-to-nearest is monotone, so
//   fl(p - q) >= fl(lo - q) >= 0; likewise on the right; inside, the gap is 0.  Squaring non-negative values and the two
//   additions are monotone under round-to-nearest too.  Hence  bound(q, box) <= d2(q, p)  for EVERY point p of the box, as
//   computed binary32 values -- and the same with a whole box of queries on the left (box-to-box: lo_B - hi_A <= p - q).
// A box (for one lane) or a chunk (for the whole workgroup) is therefore skipped exactly when its bound is >= the current
// third-best: nothing in it can enter the three smallest values as a strictly smaller one, and an equal one would leave the
// multiset of values unchanged.  With >= a cloud of duplicates (third-best 0 after the own chunk) costs one pass.
// Points that are not finite never enter: their d2 is +inf or NaN, and neither is < a third-best that starts at +inf.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sum_sq(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }
__device__ __forceinline__ float gap(float lo, float hi, float q_lo, float q_hi) { return fmaxf(fmaxf(lo - q_hi, q_lo - hi), 0.0f); }

__device__ __forceinline__ void keep3(float d2, float& b0, float& b1, float& b2)
{
    if (d2 < b2) {
        if (d2 < b1) {
            b2 = b1;
            if (d2 < b0) {
                b1 = b0;
                b0 = d2;
            } else {
                b1 = d2;
            }
        } else {
            b2 = d2;
        }
    }
}

// one staged chunk against one query (`skip`: the query's own slot in its own chunk, -1 elsewhere)
__device__ __forceinline__ void scan_chunk(const float4* s_pts, float qx, float qy, float qz, int skip, float& b0, float& b1, float& b2)
{
#pragma unroll 8
    for (int j = 0; j < kKnnChunk; ++j) {
        const float4 p  = s_pts[j]; // one address for the whole wave: an LDS broadcast
        const float  d2 = sum_sq(qx - p.x, qy - p.y, qz - p.z);
        if (j != skip) keep3(d2, b0, b1, b2);
    }
}
// the largest value of `v` over the workgroup (every thread gets it; one barrier)
__device__ __forceinline__ float block_max(float v, float* s_wave_max)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) s_wave_max[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_wave_max[0], s_wave_max[1]), fmaxf(s_wave_max[2], s_wave_max[3]));
}

__global__ void __launch_bounds__(kKnnChunk) k_knn_query(int64_t n, uint32_t num_chunks, const float4* __restrict__ sorted,
                                                         const float4* __restrict__ boxes, const KnnGrid* __restrict__ grid,
                                                         float* __restrict__ dist2)
{
    __shared__ float4   s_pts[kKnnChunk];
    __shared__ float    s_cand_bound[kKnnChunk];
    __shared__ uint32_t s_cand_chunk[kKnnChunk];
    __shared__ uint32_t s_wave_cnt[kKnnChunk / 64];
    __shared__ float    s_wave_max[kKnnChunk / 64];
    const int      t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t own  = blockIdx.x;
    const int64_t  gi   = (int64_t)own * kKnnChunk + t;
    // (slots behind the last point read the last point and turn NaN: never a neighbour, never a query)
    float4 me = sorted[gi < n ? gi : n - 1];
    if (gi >= n) me.x = me.y = me.z = NAN;
    const bool     valid = finite3(me.x, me.y, me.z);
    // (a lane without a query holds zeros: it never scans and never raises the workgroup's bound)
    float b0 = valid ? INFINITY : 0.0f, b1 = b0, b2 = b0;

    // ---- the own chunk, brute force (j != i by index: coincident points are each other's neighbours at distance 0)
    s_pts[t] = me;
    __syncthreads();
    if (valid) scan_chunk(s_pts, me.x, me.y, me.z, t, b0, b1, b2);
    float wg_third = block_max(b2, s_wave_max); // the workgroup's largest third-best

    // ---- the other chunks, outward along the curve: candidate k = 0, 1, 2, ... is chunk own - 1, own + 1, own - 2, ...
    const float4   q_lo = boxes[2 * (int64_t)own], q_hi = boxes[2 * (int64_t)own + 1];
    const uint32_t reach = own > num_chunks - 1 - own ? own : num_chunks - 1 - own;
    const uint64_t k_end = 2ull * reach;
    for (uint64_t k0 = 0; k0 < k_end; k0 += kKnnChunk) {
        if (wg_third == 0.0f) break; // every bound is >= 0: nothing is left to find
        // one candidate box per lane against the workgroup's bound; the survivors, in outward order, into LDS
        const uint64_t k    = k0 + t;
        bool           cand = false;
        float          bound = 0.0f;
        uint32_t       c = 0;
        if (k < k_end) {
            const int64_t d  = (int64_t)(k >> 1) + 1;
            const int64_t cc = (k & 1) ? (int64_t)own + d : (int64_t)own - d;
            if (cc >= 0 && cc < (int64_t)num_chunks) {
                c               = (uint32_t)cc;
                const float4 lo = boxes[2 * cc], hi = boxes[2 * cc + 1];
                bound = sum_sq(gap(lo.x, hi.x, q_lo.x, q_hi.x), gap(lo.y, hi.y, q_lo.y, q_hi.y), gap(lo.z, hi.z, q_lo.z, q_hi.z));
                cand  = bound < wg_third;
            }
        }
        const uint64_t mask = __ballot(cand);
        if (lane == 0) s_wave_cnt[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kKnnChunk / 64; ++w) {
            before += w < wave ? s_wave_cnt[w] : 0u;
            total += s_wave_cnt[w];
        }
        if (cand) {
            const uint32_t slot = before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            s_cand_chunk[slot]  = c;
            s_cand_bound[slot]  = bound;
        }
        __syncthreads();
        for (uint32_t e = 0; e < total; ++e) {
            if (!(s_cand_bound[e] < wg_third)) continue; // the bound has tightened since the test (uniform)
            const uint32_t cc = s_cand_chunk[e];
            const int64_t  g  = (int64_t)cc * kKnnChunk + t;
            float4         p  = sorted[g < n ? g : n - 1];
            if (g >= n) p.x = p.y = p.z = NAN;
            s_pts[t] = p;
            const float4 lo = boxes[2 * (int64_t)cc], hi = boxes[2 * (int64_t)cc + 1];
            __syncthreads();
            const float mine = sum_sq(gap(lo.x, hi.x, me.x, me.x), gap(lo.y, hi.y, me.y, me.y), gap(lo.z, hi.z, me.z, me.z));
            if (mine < b2) scan_chunk(s_pts, me.x, me.y, me.z, -1, b0, b1, b2);
            wg_third = block_max(b2, s_wave_max); // (its barrier also ends every wave's reads of s_pts before the next chunk is staged)
        }
        __syncthreads(); // the candidate list is rewritten by the next round
    }

    if (gi < n) {
        const uint32_t others = grid->num_valid > 0 ? grid->num_valid - 1 : 0;
        float          r      = 0.0f;
        if (valid) {
            if (others >= 3) r = ((b0 + b1) + b2) / 3.0f;
            else if (others == 2) r = (b0 + b1) / 2.0f;
            else if (others == 1) r = b0;
        }
        dist2[__float_as_uint(me.w)] = r;
    }
}

// ---- the rows of 3DGS's create_from_pcd, one thread per point of the caller's order / per coefficient
__global__ void __launch_bounds__(256) k_init_rows(int64_t n, const float* pos /* may be raw_pos */, const float* __restrict__ dist2,
                                                   float min_dist2, float raw_opacity, float* raw_pos, float* __restrict__ raw_scale,
                                                   float* __restrict__ raw_rotq, float* __restrict__ raw_opac, float* act_pos,
                                                   float* __restrict__ act_scale, float* __restrict__ act_rotq,
                                                   float* __restrict__ act_opac)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
    raw_pos[3 * i] = x, raw_pos[3 * i + 1] = y, raw_pos[3 * i + 2] = z;
    if (act_pos != raw_pos) act_pos[3 * i] = x, act_pos[3 * i + 1] = y, act_pos[3 * i + 2] = z;
    const float s = logf(sqrtf(fmaxf(dist2[i], min_dist2))), es = act_exp(s);
    for (int c = 0; c < 3; ++c) {
        raw_scale[3 * i + c] = s;
        act_scale[3 * i + c] = es;
    }
    const float4 q = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    reinterpret_cast<float4*>(raw_rotq)[i] = q;
    reinterpret_cast<float4*>(act_rotq)[i] = q;
    raw_opac[i] = raw_opacity;
    act_opac[i] = act_sigmoid(raw_opacity);
}

__global__ void __launch_bounds__(256) k_init_sh(int64_t total, int sh_floats, const float* __restrict__ rgb, float* raw_sh,
                                                 float* act_sh)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / sh_floats;
        const int     c = (int)(e - r * sh_floats);
        const float   v = c < 3 ? (rgb[3 * r + c] - 0.5f) / 0.28209479177387814f : 0.0f; // RGB2SH; the higher bands start at 0
        raw_sh[e] = v;
        if (act_sh != raw_sh) act_sh[e] = v;
    }
}

} // namespace

size_t knn_box_partial_bytes() { return sizeof(BoxPartial) * kBoxBlocks; }

void launch_knn_grid(int64_t n, const float* pos, void* partial, KnnGrid* grid, hipStream_t stream)
{
    int64_t blocks = (n + 255) / 256;
    if (blocks > kBoxBlocks) blocks = kBoxBlocks;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_knn_box_partial, dim3((unsigned)blocks), dim3(256), 0, stream, n, pos, reinterpret_cast<BoxPartial*>(partial));
    hipLaunchKernelGGL(k_knn_box_finish, dim3(1), dim3(256), 0, stream, (int)blocks, reinterpret_cast<const BoxPartial*>(partial), grid);
}

void launch_knn_gather_boxes(int64_t n, const float* pos, const uint32_t* perm, float4* sorted, float4* boxes, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_knn_gather_boxes, dim3((unsigned)((n + kKnnChunk - 1) / kKnnChunk)), dim3(kKnnChunk), 0, stream, n, pos, perm,
                       sorted, boxes);
}

void launch_knn_query(int64_t n, const float4* sorted, const float4* boxes, const KnnGrid* grid, float* dist2, hipStream_t stream)
{
    if (n <= 0) return;
    const uint32_t chunks = (uint32_t)((n + kKnnChunk - 1) / kKnnChunk);
    hipLaunchKernelGGL(k_knn_query, dim3(chunks), dim3(kKnnChunk), 0, stream, n, chunks, sorted, boxes, grid, dist2);
}

void launch_init_rows(int64_t n, int sh_floats, const float* pos, const float* rgb, const float* dist2, float min_dist2,
                      float raw_opacity, const AdamArrays& raw, const AdamArrays& act, hipStream_t stream)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_init_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, pos, dist2, min_dist2, raw_opacity,
                       raw.pos, raw.scale, raw.rotq, raw.opacity, act.pos, act.scale, act.rotq, act.opacity);
    const int64_t total = n * sh_floats;
    hipLaunchKernelGGL(k_init_sh, dim3(grid_256(total)), dim3(256), 0, stream, total, sh_floats, rgb, raw.sh, act.sh);
}

} // namespace lcgs

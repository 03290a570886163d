// tsdf.hip -- a surface out of the trained scene (no reference counterpart; include/lcgs_hip.h has the definitions):
//   integrate   Curless & Levoy's running mean of the truncated projective distance, nearest-pixel lookup.  One lane owns one
//               sample, 64 consecutive samples of a lattice row per wave (coalesced 4-byte state, 12-byte colour): the state is
//               loaded once per launch, run through up to kTsdfViewChunk views in registers and stored once, and only where a view
//               touched it.  The views are looped inside the kernel from a table in the kernel's arguments that every lane reads
//               uniformly (scalar loads); a view none of the wave's samples projects into is skipped for the whole wave (whole
//               rows behind a camera or beside its frustum are the common case).  The maps are gathered straight from memory:
//               nearest-pixel reads of maps that fit the Infinity Cache.  Streaming accesses for the once-per-launch state.
//   mesh        marching tetrahedra on the 6-tetrahedron Kuhn split.  A cell's 19 distinct edges are the pairs of corners whose
//               offset codes are comparable as bit sets, each keyed by (lower sample, direction): the cell pass ORs the crossing
//               ones into a 7-bit mask per LOWER sample (integer OR: order-free), so a vertex's id is the exclusive sum of the
//               masks' popcounts below its sample plus the rank of its bit -- welded without a sort or a hash.  The triangle pass
//               recomputes each tetrahedron's sign case and looks its vertices' ids up.
#include "launch.hpp"
#include "stream_access.hpp"

namespace lcgs
{
namespace
{

__device__ __forceinline__ float lattice_pos(float origin, float voxel, int i) { return origin + voxel * (float)i; }

// ---- integrate
__global__ void __launch_bounds__(256) k_tsdf_integrate(TsdfGrid g, float* __restrict__ tsdf, float* __restrict__ weight,
                                                        float* __restrict__ rgb, float trunc, float depth_max, float alpha_min,
                                                        int num_views, TsdfViews views)
{
    const int     xchunks = (g.nx + 63) >> 6;
    const int64_t tasks   = (int64_t)xchunks * g.ny * g.nz; // 64 samples of one lattice row each
    const int     lane    = threadIdx.x & 63;
    for (int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); task < tasks; task += (int64_t)gridDim.x * 4) {
        const int64_t row  = task / xchunks;
        const int     i    = (int)(task - row * xchunks) * 64 + lane;
        const int     k    = (int)(row / g.ny), j = (int)(row - (int64_t)k * g.ny);
        const bool    live = i < g.nx;
        const int64_t s    = row * g.nx + i;
        const float   X0 = lattice_pos(g.origin[0], g.voxel, i), X1 = lattice_pos(g.origin[1], g.voxel, j),
                      X2 = lattice_pos(g.origin[2], g.voxel, k);
        float t = 0.0f, w = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
        if (live) {
            t = ld_stream(tsdf + s), w = ld_stream(weight + s);
            if (rgb) c0 = ld_stream(rgb + 3 * s), c1 = ld_stream(rgb + 3 * s + 1), c2 = ld_stream(rgb + 3 * s + 2);
        }
        bool touched = false;
        for (int n = 0; n < num_views; ++n) {
            const TsdfView& v = views.v[n]; // uniform: scalar loads, once per view and wave
            // gs_math.hpp view_transform, same operation order
            const float vx = v.right[0] * X0 + v.right[1] * X1 + v.right[2] * X2 + v.tx;
            const float vy = v.up[0] * X0 + v.up[1] * X1 + v.up[2] * X2 + v.ty;
            const float z  = v.front[0] * X0 + v.front[1] * X1 + v.front[2] * X2 + v.tz;
            const float fw = (float)v.W, fh = (float)v.H;
            const float ux = ((vx / z) * v.inv_tanx + 1.0f) * (0.5f * fw);
            const float uy = ((vy / z) * v.inv_tany + 1.0f) * (0.5f * fh);
            // a NaN fails every comparison: skipped
            const bool in = live && z > 0.0f && ux >= 0.0f && ux < fw && uy >= 0.0f && uy < fh;
            if (__ballot(in) == 0ull) continue; // no sample of the wave projects into the view
            if (!in) continue;
            const int64_t pix = (int64_t)(int)floorf(uy) * v.W + (int)floorf(ux);
            float         d   = v.depth[pix];
            if (v.alpha) {
                const float a = v.alpha[pix];
                if (!(a >= alpha_min)) continue;
                d = d / a;
            }
            if (!(d > 0.0f && d <= depth_max)) continue; // (not finite: +inf fails the second test, a NaN both)
            const float sdf = d - z;
            if (sdf < -trunc) continue;
            const float u  = fminf(1.0f, sdf / trunc);
            const float w1 = w + 1.0f;
            t              = (t * w + u) / w1;
            if (rgb && v.image) {
                const int64_t plane = (int64_t)v.W * v.H;
                c0 = (c0 * w + v.image[pix]) / w1;
                c1 = (c1 * w + v.image[plane + pix]) / w1;
                c2 = (c2 * w + v.image[2 * plane + pix]) / w1;
            }
            w       = w1;
            touched = true;
        }
        if (touched) {
            st_stream(tsdf + s, t), st_stream(weight + s, w);
            if (rgb) st_stream(rgb + 3 * s, c0), st_stream(rgb + 3 * s + 1, c1), st_stream(rgb + 3 * s + 2, c2);
        }
    }
}

// ---- mesh
// the sample at corner `code` (dx + 2 dy + 4 dz) of the cell whose lowest corner is sample s
__device__ __forceinline__ int64_t corner(const TsdfGrid& g, int64_t s, int code)
{
    return s + (code & 1) + ((code >> 1) & 1) * (int64_t)g.nx + ((code >> 2) & 1) * (int64_t)g.nx * g.ny;
}
// (i, j, k) of sample s; true iff s is the lowest corner of a cell
__device__ __forceinline__ bool cell_of(const TsdfGrid& g, int64_t s, int& i, int& j, int& k)
{
    const int64_t row = s / g.nx;
    i = (int)(s - row * g.nx), k = (int)(row / g.ny), j = (int)(row - (int64_t)k * g.ny);
    return i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1;
}
// bit c: corner c of the cell at s is inside (tsdf < 0: neither -0.0f nor a NaN)
__device__ __forceinline__ uint32_t inside_bits(const TsdfGrid& g, const float* __restrict__ tsdf, int64_t s)
{
    uint32_t in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) in |= (uint32_t)(tsdf[corner(g, s, c)] < 0.0f) << c;
    return in;
}
// tetrahedron q of the Kuhn split, the q-th permutation (a, b, c) of the axes in lexicographic order: the corner codes
// c0 = 0, c1 = 1 << a, c2 = c1 | 1 << b, c3 = 7, four bits each; odd permutations are negatively oriented
__device__ __forceinline__ uint32_t tet_codes(int q)
{
    const int a = q >> 1, b = (0x102021 >> (4 * q)) & 3; // b of (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0) = 1 2 0 2 0 1
    const uint32_t c1 = 1u << a, c2 = c1 | (1u << b);
    return c1 << 4 | c2 << 8 | 7u << 12;
}
__device__ __forceinline__ bool tet_negative(int q) { return (0x26 >> q) & 1; } // q = 1, 2, 5
__device__ __forceinline__ uint32_t tet_inside(uint32_t in, uint32_t codes)
{
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) m |= ((in >> ((codes >> (4 * i)) & 7)) & 1u) << i;
    return m;
}

__global__ void __launch_bounds__(256) k_tsdf_mesh_cells(TsdfGrid g, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                         float weight_min, uint32_t* __restrict__ word)
{
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += (int64_t)gridDim.x * 256) {
        int i, j, k;
        if (!cell_of(g, s, i, j, k)) continue;
        bool valid = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) valid = valid && weight[corner(g, s, c)] >= weight_min; // (a NaN weight: not valid)
        if (!valid) continue;
        const uint32_t in = inside_bits(g, tsdf, s);
        if (in == 0u || in == 255u) continue;
        uint32_t count = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int nin = __popc(tet_inside(in, tet_codes(q)));
            count += nin == 2 ? 2u : ((nin == 1 || nin == 3) ? 1u : 0u);
        }
        // the cell's edges: lower corner c, direction d disjoint from c
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            uint32_t m = c == 0 ? count << 8 : 0u;
#pragma unroll
            for (int d = 1; d < 8; ++d)
                if ((c & d) == 0) m |= (((in >> c) ^ (in >> (c | d))) & 1u) << (d - 1);
            if (m) atomicOr(word + corner(g, s, c), m);
        }
    }
}

__global__ void __launch_bounds__(256) k_tsdf_mesh_counts(int64_t n, const uint32_t* __restrict__ word, uint32_t* __restrict__ vcount,
                                                          uint32_t* __restrict__ tcount, unsigned long long* __restrict__ totals)
{
    __shared__ unsigned long long s_sum[2][4];
    unsigned long long            nv = 0, nt = 0;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += (int64_t)gridDim.x * 256) {
        const uint32_t w = word[s], v = __popc(w & 0x7Fu), t = (w >> 8) & 0xFu;
        vcount[s] = v, tcount[s] = t;
        nv += v, nt += t;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nv += __shfl_down(nv, off, 64), nt += __shfl_down(nt, off, 64);
    if ((threadIdx.x & 63) == 0) s_sum[0][threadIdx.x >> 6] = nv, s_sum[1][threadIdx.x >> 6] = nt;
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long sum = s_sum[threadIdx.x][0] + s_sum[threadIdx.x][1] + s_sum[threadIdx.x][2] + s_sum[threadIdx.x][3];
        if (sum) atomicAdd(totals + threadIdx.x, sum);
    }
}

__global__ void __launch_bounds__(256) k_tsdf_mesh_vertices(TsdfGrid g, const float* __restrict__ tsdf, const float* __restrict__ rgb,
                                                            const uint32_t* __restrict__ word, const uint32_t* __restrict__ vincl,
                                                            float* __restrict__ vertices, float* __restrict__ vertex_rgb)
{
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += (int64_t)gridDim.x * 256) {
        const uint32_t mask = word[s] & 0x7Fu;
        if (!mask) continue;
        int i, j, k;
        cell_of(g, s, i, j, k);
        int64_t     id = (int64_t)vincl[s] - __popc(mask);
        const float ta = tsdf[s];
        const float Xa[3] = { lattice_pos(g.origin[0], g.voxel, i), lattice_pos(g.origin[1], g.voxel, j),
                              lattice_pos(g.origin[2], g.voxel, k) };
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (!((mask >> (d - 1)) & 1u)) continue;
            const int64_t sb     = corner(g, s, d);
            const float   tb     = tsdf[sb];
            const float   lambda = ta / (ta - tb);
            const float   Xb[3]  = { lattice_pos(g.origin[0], g.voxel, i + (d & 1)), lattice_pos(g.origin[1], g.voxel, j + ((d >> 1) & 1)),
                                     lattice_pos(g.origin[2], g.voxel, k + ((d >> 2) & 1)) };
#pragma unroll
            for (int c = 0; c < 3; ++c) vertices[3 * id + c] = Xa[c] + lambda * (Xb[c] - Xa[c]);
            if (vertex_rgb) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float ca = rgb[3 * s + c], cb = rgb[3 * sb + c];
                    vertex_rgb[3 * id + c] = ca + lambda * (cb - ca);
                }
            }
            ++id;
        }
    }
}

struct MeshIds {
    const TsdfGrid&                g;
    const uint32_t* __restrict__   word;
    const uint32_t* __restrict__   vincl;
    int64_t                        s;
    uint32_t                       codes;
    // the id of the vertex on the edge between corners i and j of the tetrahedron
    __device__ __forceinline__ uint32_t operator()(int i, int j) const
    {
        const int      lo = i < j ? i : j, hi = i < j ? j : i;
        const uint32_t cl = (codes >> (4 * lo)) & 7u, dir = ((codes >> (4 * hi)) & 7u) ^ cl;
        const int64_t  sl = corner(g, s, (int)cl);
        const uint32_t m  = word[sl] & 0x7Fu;
        return vincl[sl] - __popc(m) + __popc(m & ((1u << (dir - 1)) - 1u));
    }
};
// (a, b, c) rotated so that the lowest id comes first
__device__ __forceinline__ void store_triangle(uint32_t* __restrict__ out, uint32_t a, uint32_t b, uint32_t c)
{
    if (b < a && b < c) {
        const uint32_t t = a;
        a = b, b = c, c = t;
    } else if (c < a && c < b) {
        const uint32_t t = c;
        c = b, b = a, a = t;
    }
    out[0] = a, out[1] = b, out[2] = c;
}

__global__ void __launch_bounds__(256) k_tsdf_mesh_triangles(TsdfGrid g, const float* __restrict__ tsdf, const uint32_t* __restrict__ word,
                                                             const uint32_t* __restrict__ vincl, const uint32_t* __restrict__ tincl,
                                                             uint32_t* __restrict__ triangles)
{
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += (int64_t)gridDim.x * 256) {
        const uint32_t count = (word[s] >> 8) & 0xFu;
        if (!count) continue;
        const uint32_t in = inside_bits(g, tsdf, s);
        uint32_t*      out = triangles + 3 * ((int64_t)tincl[s] - count);
        for (int q = 0; q < 6; ++q) {
            const uint32_t codes = tet_codes(q);
            const uint32_t ins   = tet_inside(in, codes);
            const int      nin   = __popc(ins);
            if (nin == 0 || nin == 4) continue;
            const MeshIds id{ g, word, vincl, s, codes };
            const bool    neg = tet_negative(q);
            if (nin != 2) {
                // corner p alone on its side: the triangle on its three edges, in the order of the other corners, has its normal
                // pointing away from p iff the tetrahedron's orientation times (-1)^p is positive
                uint32_t  rest = nin == 1 ? ins : (~ins & 15u);
                const int p    = __ffs(rest) - 1;
                rest           = 15u ^ (1u << p);
                const int q1 = __ffs(rest) - 1;
                rest &= rest - 1;
                const int q2 = __ffs(rest) - 1;
                rest &= rest - 1;
                const int      q3 = __ffs(rest) - 1;
                const uint32_t a = id(p, q1), b = id(p, q2), c = id(p, q3);
                const bool     away = ((p & 1) != 0) == neg;
                if (away == (nin == 1)) store_triangle(out, a, b, c);
                else store_triangle(out, a, c, b);
                out += 3;
            } else {
                // inside p0 < p1, outside q0 < q1: the cycle (p0 q0) (p0 q1) (p1 q1) (p1 q0) points from inside to outside iff
                // the tetrahedron (p0, p1, q0, q1) is positively oriented: the parity of p0 + p1 - 1 against the tetrahedron's
                const int p0 = __ffs(ins) - 1, p1 = 31 - __clz(ins);
                const uint32_t outs = ~ins & 15u;
                const int      q0 = __ffs(outs) - 1, q1 = 31 - __clz(outs);
                uint32_t       w0 = id(p0, q0), w1 = id(p0, q1), w2 = id(p1, q1), w3 = id(p1, q0);
                if ((((p0 + p1) & 1) == 0) != neg) {
                    const uint32_t t = w1;
                    w1 = w3, w3 = t;
                }
                // the lowest id first, the cycle kept
                for (int r = 0; r < 3 && !(w0 < w1 && w0 < w2 && w0 < w3); ++r) {
                    const uint32_t t = w0;
                    w0 = w1, w1 = w2, w2 = w3, w3 = t;
                }
                // (w0 w1 w2) and (w0 w2 w3): ordered by their other two ids, each pair sorted
                const uint32_t a_lo = min(w1, w2), a_hi = max(w1, w2), b_lo = min(w2, w3), b_hi = max(w2, w3);
                const bool     a_first = a_lo < b_lo || (a_lo == b_lo && a_hi < b_hi);
                uint32_t *first = a_first ? out : out + 3, *second = a_first ? out + 3 : out;
                first[0] = w0, first[1] = w1, first[2] = w2;
                second[0] = w0, second[1] = w2, second[2] = w3;
                out += 6;
            }
        }
    }
}

} // namespace

void launch_tsdf_integrate(const TsdfGrid& g, float* tsdf, float* weight, float* rgb, float trunc, float depth_max, float alpha_min,
                           int num_views, const TsdfViews& views, hipStream_t stream)
{
    const int64_t tasks = (int64_t)((g.nx + 63) / 64) * g.ny * g.nz;
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(grid_256(tasks * 64)), dim3(256), 0, stream, g, tsdf, weight, rgb, trunc, depth_max,
                       alpha_min, num_views, views);
}

void launch_tsdf_mesh_cells(const TsdfGrid& g, const float* tsdf, const float* weight, float weight_min, uint32_t* word,
                            hipStream_t stream)
{
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    hipLaunchKernelGGL(k_tsdf_mesh_cells, dim3(grid_256(n)), dim3(256), 0, stream, g, tsdf, weight, weight_min, word);
}

void launch_tsdf_mesh_counts(int64_t n, const uint32_t* word, uint32_t* vcount, uint32_t* tcount, unsigned long long* totals,
                             hipStream_t stream)
{
    // a few blocks per CU: two atomics each
    const unsigned blocks = grid_256(n) < 2048u ? grid_256(n) : 2048u;
    hipLaunchKernelGGL(k_tsdf_mesh_counts, dim3(blocks), dim3(256), 0, stream, n, word, vcount, tcount, totals);
}

void launch_tsdf_mesh_vertices(const TsdfGrid& g, const float* tsdf, const float* rgb, const uint32_t* word, const uint32_t* vincl,
                               float* vertices, float* vertex_rgb, hipStream_t stream)
{
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    hipLaunchKernelGGL(k_tsdf_mesh_vertices, dim3(grid_256(n)), dim3(256), 0, stream, g, tsdf, rgb, word, vincl, vertices, vertex_rgb);
}

void launch_tsdf_mesh_triangles(const TsdfGrid& g, const float* tsdf, const uint32_t* word, const uint32_t* vincl,
                                const uint32_t* tincl, uint32_t* triangles, hipStream_t stream)
{
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;
    hipLaunchKernelGGL(k_tsdf_mesh_triangles, dim3(grid_256(n)), dim3(256), 0, stream, g, tsdf, word, vincl, tincl, triangles);
}

} // namespace lcgs

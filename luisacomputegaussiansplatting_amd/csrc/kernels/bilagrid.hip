// bilagrid.hip -- per-view bilateral-grid colour correction ("Bilateral Guided Radiance Field Processing"): the slice of a
// [12][L][GH][GW] grid of 3 x 4 affine transforms at (pixel x, pixel y, luminance of the input pixel) applied to the input colour,
// its two gradients, and the total-variation term of a set of grids.  The definition is the contract in include/lcgs_hip.h;
// DESIGN.md 9 has what bounds each kernel.  All binary32 expressions are uncontracted (-ffp-contract=off) and written as the
// header writes them; no float atomics anywhere: the same inputs give the same bits.
//
//   k_bilagrid_pixels<GRAD>  one workgroup per 32 x 16 pixel tile, two pixels a lane.  The tile's pixels fall into few xy cells of
//       the grid (2 x 2 vertex columns at 1080p under 16 x 16 x 8, 3 x 3 across a cell boundary), and every lane needs 8 corners x
//       12 channels at a z of its own: in the tensor's channel-major layout 96 scattered loads.  So the workgroup stages the
//       vertex columns its pixels can touch into LDS transposed to [vertex][l][12] -- a corner's 12 channels are 48 consecutive
//       bytes -- and samples from there.  Budget: kStageFloats * 4 = 16 KiB a workgroup: eight 4-wave workgroups, a CU's 32 wave
//       slots, take 128 of the 160 KiB, so LDS never bounds the occupancy (the registers do: 76 / 90 VGPRs, 6 / 5 waves a SIMD).
//       A tile whose footprint is larger (a tiny image under a large grid: 5 x 7 pixels under 16 x 16 x 8 touch 14 x 14 columns)
//       samples from global memory instead; the branch is uniform per workgroup.  GRAD = false writes the slice, GRAD = true
//       dL/dimg.
//   dL/dgrid is a GATHER.  The trilinear weight is a product of hat functions, so vertex (i, j, .) receives from the pixel
//       rectangle |x - i| < 1, |y - j| < 1 (computed in binary64 with a pixel to spare on every side: a superset; the weight is the
//       forward's own expression, 0 off the support).  Grids with few vertices split every footprint into `slices` row bands (a
//       function of the dimensions only), one binary64 partial each in the context's loss workspace, summed in slice order by
//       k_bilagrid_grid_combine.  Vertices nothing reaches are written as exact zeros.  Two shapes, both measured
//       (profiles/bilagrid_bench.txt):
//   k_bilagrid_column_grad<8>  L <= 8: one workgroup per vertex COLUMN (i, j) and row slice.  A lane keeps 8 x 12 binary32 sums,
//       statically indexed, and visits a pixel once for all levels; the workgroup's sums run in binary64 in a fixed order.
//   k_bilagrid_grid_grad     deeper grids: one workgroup per vertex (i, j, l) and row slice.  A lane keeps 12 binary64 sums and
//       skips pixels whose z cell does not touch l; the workgroup reduces them in a fixed order (wave butterfly, then the four
//       waves in order).  Works for any L, but visits every pixel 4 L times.
//   k_bilagrid_tv<GRAD>      one lane per grid element: its forward differences squared into the loss (binary64, one partial per
//       workgroup, the finish step of ordered_sum.hpp), its <= 6 neighbours gathered into the gradient.
#include "launch.hpp"
#include "ordered_sum.hpp"
#include "stream_access.hpp"

namespace lcgs
{
namespace
{
constexpr int kTW = kBilagridTileW, kTH = kBilagridTileH;
constexpr int kThreads     = 256;
constexpr int kStageFloats = 4096; // 16 KiB of staged vertex columns a workgroup
static_assert(kThreads == kOrderedSumThreads, "the finish step runs with this workgroup size");
static_assert(kTW * kTH == 2 * kThreads, "two pixels a lane");

struct Coord {
    int   v0; // the lower vertex of the cell
    float f;  // the position inside it, [0, 1) (1 only at z = L - 1)
};
// x = ((float)p + 0.5f) / n * (g - 1), x0 = min(floor(x), g - 2): non-decreasing in p, 0 <= x0 <= g - 2
__device__ __forceinline__ Coord pixel_coord(int p, int n, int g)
{
    const float x  = ((float)p + 0.5f) / (float)n * (float)(g - 1);
    int         x0 = (int)x; // x > 0
    if (x0 > g - 2) x0 = g - 2;
    return { x0, x - (float)x0 };
}
struct Guide {
    Coord z;
    bool  inside; // 0 < zr < L - 1: the guidance passes a gradient
};
__device__ __forceinline__ Guide guidance(float r, float g, float b, int L)
{
    const float gray = (0.299f * r + 0.587f * g) + 0.114f * b;
    const float top  = (float)(L - 1);
    const float zr   = gray * top;
    const float z    = fminf(fmaxf(zr, 0.0f), top); // (NaN -> 0: every index stays inside the grid)
    int         z0   = (int)z;
    if (z0 > L - 2) z0 = L - 2;
    return { { z0, z - (float)z0 }, zr > 0.0f && zr < top };
}

// a corner's 12 channels: from the staged columns, [vertex][l][12] ...
struct StagedColumns {
    const float* s;
    int          nvx, L, vx, vy; // vx, vy: the pixel's cell inside the staged block
    __device__ __forceinline__ void corner(int dx, int dy, int l, float (&v)[12]) const
    {
        const float* p = s + ((size_t)(((vy + dy) * nvx + (vx + dx)) * L + l)) * 12;
#pragma unroll
        for (int c = 0; c < 12; ++c) v[c] = p[c];
    }
};
// ... or from the tensor, [12][L][GH][GW]
struct GlobalColumns {
    const float* g;
    int          GW, GH, L, x0, y0;
    __device__ __forceinline__ void corner(int dx, int dy, int l, float (&v)[12]) const
    {
        const int64_t plane = (int64_t)GH * GW, o = (int64_t)l * plane + (int64_t)(y0 + dy) * GW + (x0 + dx);
#pragma unroll
        for (int c = 0; c < 12; ++c) v[c] = g[(int64_t)c * L * plane + o];
    }
};

// the xy-bilinear sample of level l as nested lerps a + t (b - a): along x, then y
template <class Columns>
__device__ __forceinline__ void sample_level(const Columns& col, int l, float fx, float fy, float (&A)[12])
{
    float v00[12], v10[12], v01[12], v11[12];
    col.corner(0, 0, l, v00);
    col.corner(1, 0, l, v10);
    col.corner(0, 1, l, v01);
    col.corner(1, 1, l, v11);
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        const float a = v00[c] + fx * (v10[c] - v00[c]);
        const float b = v01[c] + fx * (v11[c] - v01[c]);
        A[c]          = a + fy * (b - a);
    }
}

template <bool GRAD, class Columns>
__device__ __forceinline__ void pixel(const Columns& col, float fx, float fy, const Guide& gd, int L, float r, float g, float b,
                                      int64_t o, int64_t plane, const float* __restrict__ dL_dout, float* __restrict__ out)
{
    float A0[12], A1[12];
    sample_level(col, gd.z.v0, fx, fy, A0);
    sample_level(col, gd.z.v0 + 1, fx, fy, A1);
    const float fz = gd.z.f;
    if (!GRAD) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float A[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) A[m] = A0[4 * k + m] + fz * (A1[4 * k + m] - A0[4 * k + m]);
            st_stream(out + k * plane + o, ((A[0] * r + A[1] * g) + A[2] * b) + A[3]);
        }
    } else {
        const float g0 = dL_dout[o], g1 = dL_dout[plane + o], g2 = dL_dout[2 * plane + o];
        const float gr[3] = { g0, g1, g2 };
        // through the guidance: sum_r g_r (dA[4r .. 4r+3] . (r, g, b, 1)), dA = the level above minus the level below
        float through = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d0 = A1[4 * k] - A0[4 * k], d1 = A1[4 * k + 1] - A0[4 * k + 1], d2 = A1[4 * k + 2] - A0[4 * k + 2],
                        d3 = A1[4 * k + 3] - A0[4 * k + 3];
            through += gr[k] * (((d0 * r + d1 * g) + d2 * b) + d3);
        }
        through = gd.inside ? through * (float)(L - 1) : 0.0f;
        const float w[3] = { 0.299f, 0.587f, 0.114f };
#pragma unroll
        for (int k = 0; k < 3; ++k) { // dL/dc_k = sum_r A[4r + k] g_r + w_k (L - 1) inside (...)
            float direct = 0.0f;
#pragma unroll
            for (int m = 0; m < 3; ++m) direct += (A0[4 * m + k] + fz * (A1[4 * m + k] - A0[4 * m + k])) * gr[m];
            st_stream(out + k * plane + o, direct + w[k] * through);
        }
    }
}

template <bool GRAD>
__global__ void __launch_bounds__(kThreads) k_bilagrid_pixels(int W, int H, const float* __restrict__ grid, int GW, int GH, int L,
                                                              const float* __restrict__ img, const float* __restrict__ dL_dout,
                                                              float* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float s_cols[kStageFloats];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    // the vertex columns the tile's pixels touch: the first pixel's cell to the last pixel's cell + 1 (pixel_coord is monotone)
    const int xl = x0 + kTW - 1 < W ? x0 + kTW - 1 : W - 1, yl = y0 + kTH - 1 < H ? y0 + kTH - 1 : H - 1;
    const int ix_lo = pixel_coord(x0, W, GW).v0, iy_lo = pixel_coord(y0, H, GH).v0;
    const int nvx = pixel_coord(xl, W, GW).v0 + 2 - ix_lo, nvy = pixel_coord(yl, H, GH).v0 + 2 - iy_lo;
    const int  staged_floats = nvx * nvy * L * 12; // <= 256 * 256 * 16 * 12
    const bool staged        = staged_floats <= kStageFloats;
    if (staged) {
        const int64_t plane = (int64_t)GH * GW;
        for (int i = tid; i < staged_floats; i += kThreads) { // vx fastest: neighbouring lanes read neighbouring addresses
            const int vx = i % nvx, t1 = i / nvx, vy = t1 % nvy, t2 = t1 / nvy, l = t2 % L, c = t2 / L;
            s_cols[((vy * nvx + vx) * L + l) * 12 + c] = grid[((int64_t)c * L + l) * plane + (int64_t)(iy_lo + vy) * GW + (ix_lo + vx)];
        }
        __syncthreads();
    }
    const int64_t plane = (int64_t)W * H;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int px = x0 + (tid & 31), py = y0 + (tid >> 5) + half * (kTH / 2);
        if (px >= W || py >= H) continue;
        const int64_t o = (int64_t)py * W + px;
        const float   r = img[o], g = img[plane + o], b = img[2 * plane + o];
        const Coord   cx = pixel_coord(px, W, GW), cy = pixel_coord(py, H, GH);
        const Guide   gd = guidance(r, g, b, L);
        if (staged) {
            const StagedColumns col = { s_cols, nvx, L, cx.v0 - ix_lo, cy.v0 - iy_lo };
            pixel<GRAD>(col, cx.f, cy.f, gd, L, r, g, b, o, plane, dL_dout, out);
        } else {
            const GlobalColumns col = { grid, GW, GH, L, cx.v0, cy.v0 };
            pixel<GRAD>(col, cx.f, cy.f, gd, L, r, g, b, o, plane, dL_dout, out);
        }
    }
}

// the forward's weight of vertex `v` for a pixel whose cell starts at c.v0: 1 - f below, f above, 0 elsewhere
__device__ __forceinline__ float corner_weight(const Coord& c, int v) { return c.v0 == v ? 1.0f - c.f : (c.v0 + 1 == v ? c.f : 0.0f); }

// pixels p of an axis of n pixels with |x(p) - v| < 1, a pixel to spare on both sides, clipped to the axis: [lo, hi]
__device__ __forceinline__ void reach(int v, int n, int g, int* lo, int* hi)
{
    const double cell = (double)n / (double)(g - 1); // pixels per cell; x(p) = (p + 0.5) / cell
    const double a = (double)(v - 1) * cell - 0.5, b = (double)(v + 1) * cell - 0.5;
    const int    l = (int)floor(a) - 1, h = (int)ceil(b) + 1;
    *lo = l < 0 ? 0 : l;
    *hi = h > n - 1 ? n - 1 : h;
}

__global__ void __launch_bounds__(kThreads) k_bilagrid_grid_grad(int W, int H, int GW, int GH, int L, int slices,
                                                                 const float* __restrict__ img, const float* __restrict__ dL_dout,
                                                                 float* __restrict__ dL_dgrid, double* __restrict__ partials)
{
    __shared__ double s_red[kThreads / 64][12];
    const int tid = threadIdx.x;
    const int v = blockIdx.x, l = v % L, i = (v / L) % GW, j = v / (L * GW); // l fastest: neighbours in launch order share pixels
    int       px_lo, px_hi, py_lo, py_hi;
    reach(i, W, GW, &px_lo, &px_hi);
    reach(j, H, GH, &py_lo, &py_hi);
    const int rows = py_hi - py_lo + 1, band = (rows + slices - 1) / slices; // (rows may be <= 0: nothing in reach)
    const int row_lo = py_lo + (int)blockIdx.y * band, row_hi = row_lo + band - 1 < py_hi ? row_lo + band - 1 : py_hi;
    double    acc[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] = 0.0;
    const int64_t plane = (int64_t)W * H;
    for (int px = px_lo + (tid & 63); px <= px_hi; px += 64) {
        const float wx = corner_weight(pixel_coord(px, W, GW), i);
        if (wx == 0.0f) continue;
        for (int py = row_lo + (tid >> 6); py <= row_hi; py += kThreads / 64) {
            const float wy = corner_weight(pixel_coord(py, H, GH), j);
            if (wy == 0.0f) continue;
            const int64_t o = (int64_t)py * W + px;
            const float   r = img[o], g = img[plane + o], b = img[2 * plane + o];
            const float   wz = corner_weight(guidance(r, g, b, L).z, l);
            if (wz == 0.0f) continue;
            const double w = (double)((wx * wy) * wz);
            const double cr = (double)r, cg = (double)g, cb = (double)b;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double wg = w * (double)dL_dout[k * plane + o];
                acc[4 * k + 0] += wg * cr;
                acc[4 * k + 1] += wg * cg;
                acc[4 * k + 2] += wg * cb;
                acc[4 * k + 3] += wg;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] = wave_sum(acc[c]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 12; ++c) s_red[tid >> 6][c] = acc[c];
    }
    __syncthreads();
    if (tid < 12) {
        const double sum = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
        if (slices == 1)
            dL_dgrid[(((int64_t)tid * L + l) * GH + j) * GW + i] = (float)sum;
        else
            partials[((int64_t)blockIdx.y * gridDim.x + v) * 12 + tid] = sum;
    }
}

// The same gather with one workgroup per xy vertex COLUMN (i, j) and row slice: a lane keeps LT x 12 binary32 sums, statically
// indexed, and visits a pixel once for all levels (a pixel touches two of them; the update of a level no lane of the wave touches
// is skipped).  L <= LT.  The workgroup's sums: two levels at a time through LDS, each of 24 values as 8 interleaved runs of 32
// lanes in binary64, then the 8 runs in order.  Writes what k_bilagrid_grid_grad writes, same vertex index (j GW + i) L + l.
template <int LT>
__global__ void __launch_bounds__(kThreads) k_bilagrid_column_grad(int W, int H, int GW, int GH, int L, int slices,
                                                                   const float* __restrict__ img, const float* __restrict__ dL_dout,
                                                                   float* __restrict__ dL_dgrid, double* __restrict__ partials)
{
    constexpr int     kPitch = kThreads + 8; // 24 values x 8 runs: lane (v, run) reads bank 8 v + 8 q + run, all 64 distinct
    __shared__ float  s_part[24][kPitch];
    __shared__ double s_run[24][8];
    const int tid = threadIdx.x;
    const int col = blockIdx.x, i = col % GW, j = col / GW;
    int       px_lo, px_hi, py_lo, py_hi;
    reach(i, W, GW, &px_lo, &px_hi);
    reach(j, H, GH, &py_lo, &py_hi);
    const int rows = py_hi - py_lo + 1, band = (rows + slices - 1) / slices;
    const int row_lo = py_lo + (int)blockIdx.y * band, row_hi = row_lo + band - 1 < py_hi ? row_lo + band - 1 : py_hi;
    float     acc[LT][12];
#pragma unroll
    for (int l = 0; l < LT; ++l)
#pragma unroll
        for (int c = 0; c < 12; ++c) acc[l][c] = 0.0f;
    const int64_t plane = (int64_t)W * H;
    for (int px = px_lo + (tid & 63); px <= px_hi; px += 64) {
        const float wx = corner_weight(pixel_coord(px, W, GW), i);
        if (wx == 0.0f) continue;
        for (int py = row_lo + (tid >> 6); py <= row_hi; py += kThreads / 64) {
            const float wy = corner_weight(pixel_coord(py, H, GH), j);
            if (wy == 0.0f) continue;
            const int64_t o = (int64_t)py * W + px;
            const float   r = img[o], g = img[plane + o], b = img[2 * plane + o];
            const Coord   z = guidance(r, g, b, L).z;
            const float   wxy = wx * wy;
            float         t[12];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float wg = wxy * dL_dout[k * plane + o];
                t[4 * k + 0] = wg * r;
                t[4 * k + 1] = wg * g;
                t[4 * k + 2] = wg * b;
                t[4 * k + 3] = wg;
            }
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                const float wl = corner_weight(z, l);
                if (wl != 0.0f) {
#pragma unroll
                    for (int c = 0; c < 12; ++c) acc[l][c] = __builtin_fmaf(wl, t[c], acc[l][c]);
                }
            }
        }
    }
#pragma unroll
    for (int chunk = 0; chunk < LT / 2; ++chunk) {
        if (2 * chunk >= L) break;
#pragma unroll
        for (int v = 0; v < 24; ++v) s_part[v][tid] = acc[2 * chunk + v / 12][v % 12];
        __syncthreads();
        if (tid < 24 * 8) {
            const int v = tid >> 3, run = tid & 7;
            double    s = 0.0;
            for (int q = 0; q < kThreads / 8; ++q) s += (double)s_part[v][q * 8 + run];
            s_run[v][run] = s;
        }
        __syncthreads();
        const int l = 2 * chunk + tid / 12, c = tid % 12;
        if (tid < 24 && l < L) {
            double sum = 0.0;
#pragma unroll
            for (int run = 0; run < 8; ++run) sum += s_run[tid][run];
            if (slices == 1)
                dL_dgrid[(((int64_t)c * L + l) * GH + j) * GW + i] = (float)sum;
            else
                partials[((int64_t)blockIdx.y * gridDim.x * L + (int64_t)col * L + l) * 12 + c] = sum;
        }
    }
}

// one lane per (vertex, channel): its slices' partials in slice order
__global__ void __launch_bounds__(kThreads) k_bilagrid_grid_combine(int GW, int GH, int L, int slices,
                                                                    const double* __restrict__ partials, float* __restrict__ dL_dgrid)
{
    const int64_t vertices = (int64_t)GW * GH * L, t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= vertices * 12) return;
    double sum = 0.0;
    for (int s = 0; s < slices; ++s) sum += partials[(int64_t)s * vertices * 12 + t];
    const int v = (int)(t / 12), c = (int)(t - (int64_t)v * 12), l = v % L, i = (v / L) % GW, j = v / (L * GW);
    dL_dgrid[(((int64_t)c * L + l) * GH + j) * GW + i] = (float)sum;
}

// ---- total variation: loss = sum over axes of s_axis * sum (grid[v + e_axis] - grid[v])^2, s_axis = weight / (N count_axis)
template <bool GRAD>
__global__ void __launch_bounds__(kThreads) k_bilagrid_tv(int64_t total, int GW, int GH, int L, double sx, double sy, double sz,
                                                          const float* __restrict__ grids, float* __restrict__ dL_dgrids,
                                                          double* __restrict__ partials)
{
    __shared__ double s_red[kThreads / 64];
    const int     tid = threadIdx.x;
    const int64_t e   = (int64_t)blockIdx.x * kThreads + tid;
    double        sum = 0.0;
    if (e < total) {
        const int     i = (int)(e % GW), j = (int)((e / GW) % GH), l = (int)((e / ((int64_t)GW * GH)) % L);
        const int64_t row = GW, plane = (int64_t)GW * GH;
        const double  v = (double)grids[e];
        double        gx = 0.0, gy = 0.0, gz = 0.0;
        if (i + 1 < GW) {
            const double d = (double)grids[e + 1] - v;
            sum += sx * (d * d);
            gx -= d;
        }
        if (j + 1 < GH) {
            const double d = (double)grids[e + row] - v;
            sum += sy * (d * d);
            gy -= d;
        }
        if (l + 1 < L) {
            const double d = (double)grids[e + plane] - v;
            sum += sz * (d * d);
            gz -= d;
        }
        if (GRAD) {
            if (i > 0) gx += v - (double)grids[e - 1];
            if (j > 0) gy += v - (double)grids[e - row];
            if (l > 0) gz += v - (double)grids[e - plane];
            dL_dgrids[e] = (float)(2.0 * ((sx * gx + sy * gy) + sz * gz));
        }
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ void __launch_bounds__(kThreads) k_bilagrid_tv_finish(int64_t num, const double* __restrict__ partials,
                                                                 float* __restrict__ loss)
{
    double sum[1];
    if (sum_partials_in_order<1>(num, partials, sum)) loss[0] = (float)sum[0];
}
} // namespace

void launch_bilagrid_pixels(int W, int H, const float* grid, const BilagridDims& d, const float* img, const float* dL_dout,
                            float* out, hipStream_t stream)
{
    const dim3 wgs((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH));
    if (dL_dout)
        hipLaunchKernelGGL(k_bilagrid_pixels<true>, wgs, dim3(kThreads), 0, stream, W, H, grid, d.gw, d.gh, d.gl, img, dL_dout, out);
    else
        hipLaunchKernelGGL(k_bilagrid_pixels<false>, wgs, dim3(kThreads), 0, stream, W, H, grid, d.gw, d.gh, d.gl, img, dL_dout, out);
}

// L <= kColumnLevels: one workgroup per vertex column (k_bilagrid_column_grad); deeper grids: one per vertex
constexpr int kColumnLevels = 8;

int bilagrid_grid_slices(const BilagridDims& d)
{
    const int wgs = d.gl <= kColumnLevels ? d.gw * d.gh : d.gw * d.gh * d.gl; // <= 2^20
    if (wgs >= 1024) return 1;
    const int s = (2048 + wgs - 1) / wgs;
    return s < 64 ? s : 64;
}

size_t bilagrid_grid_partial_doubles(const BilagridDims& d)
{
    const int s = bilagrid_grid_slices(d);
    return s == 1 ? 0 : (size_t)s * d.gw * d.gh * d.gl * 12;
}

void launch_bilagrid_grid_grad(int W, int H, const BilagridDims& d, const float* img, const float* dL_dout, float* dL_dgrid,
                               double* partials, hipStream_t stream)
{
    const int slices = bilagrid_grid_slices(d), vertices = d.gw * d.gh * d.gl;
    if (d.gl <= kColumnLevels)
        hipLaunchKernelGGL(k_bilagrid_column_grad<kColumnLevels>, dim3((unsigned)(d.gw * d.gh), (unsigned)slices), dim3(kThreads), 0,
                           stream, W, H, d.gw, d.gh, d.gl, slices, img, dL_dout, dL_dgrid, partials);
    else
        hipLaunchKernelGGL(k_bilagrid_grid_grad, dim3((unsigned)vertices, (unsigned)slices), dim3(kThreads), 0, stream, W, H, d.gw,
                           d.gh, d.gl, slices, img, dL_dout, dL_dgrid, partials);
    if (slices > 1)
        hipLaunchKernelGGL(k_bilagrid_grid_combine, dim3((unsigned)((vertices * 12 + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           stream, d.gw, d.gh, d.gl, slices, partials, dL_dgrid);
}

int64_t bilagrid_tv_workgroups(int64_t num_grids, const BilagridDims& d)
{
    return (num_grids * 12 * d.gl * d.gh * d.gw + kThreads - 1) / kThreads;
}

void launch_bilagrid_tv(const float* grids, int64_t num_grids, const BilagridDims& d, double weight, float* dL_dgrids,
                        double* partials, float* loss, hipStream_t stream)
{
    const int64_t total = num_grids * 12 * d.gl * d.gh * d.gw, wgs = bilagrid_tv_workgroups(num_grids, d);
    const double  per = weight / (double)num_grids;
    const double  sx = per / (12.0 * d.gl * d.gh * (d.gw - 1)), sy = per / (12.0 * d.gl * (d.gh - 1) * d.gw),
                  sz = per / (12.0 * (d.gl - 1) * d.gh * d.gw);
    if (dL_dgrids)
        hipLaunchKernelGGL(k_bilagrid_tv<true>, dim3((unsigned)wgs), dim3(kThreads), 0, stream, total, d.gw, d.gh, d.gl, sx, sy, sz,
                           grids, dL_dgrids, partials);
    else
        hipLaunchKernelGGL(k_bilagrid_tv<false>, dim3((unsigned)wgs), dim3(kThreads), 0, stream, total, d.gw, d.gh, d.gl, sx, sy, sz,
                           grids, dL_dgrids, partials);
    hipLaunchKernelGGL(k_bilagrid_tv_finish, dim3(1), dim3(kThreads), 0, stream, wgs, partials, loss);
}
} // namespace lcgs

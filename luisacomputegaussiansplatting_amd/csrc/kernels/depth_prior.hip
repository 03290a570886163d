// depth_prior.hip -- depth-prior supervision: the Pearson-correlation loss and the aligned L1 loss of a rendered depth map
// against a depth the caller brings, with their gradients w.r.t. the depth and alpha maps (the definition is the
// contract in include/lcgs_hip.h).  No reference counterpart.
// A group is the image or one patch x patch block of a grid the caller may shift; the 32 x 16 tile grid (loss.hip's tile, one
// 256-thread workgroup each, two rows a wave) is anchored where the patch grid is, so every tile lies in one group, and the
// tiles' partial sums are stored GROUP-MAJOR: slot = group * tiles_per_group + the tile's row-major index inside its group, so
// that a group's partials are consecutive and "in slot order" is "in index order" for the image and for a patch alike.
//   pass 1  tile      (n, sum v, sum m) of the valid pixels                               -> tile1[slot]
//   pass 2  group     n, mu_v, mu_m                                                       -> rec[group]
//   pass 3  tile      the centred (sum cv^2, sum cm^2, sum cv cm); nothing read for a group that is not counted -> tile2[slot]
//   pass 4  group     var, cov, r, s, t -> rec[group]; { counted, n, 1 - r } summed over the groups in index order -> hdr = { G,
//                     N_c }, the Pearson loss, d_stats
//   pass 5  pixel     g_v and the chain to depth and alpha, every pixel of the image written once; L1: sum |res| per tile,
//                     summed in slot order -> the L1 loss.  An evaluation-only Pearson call stops in front of it; an
//                     evaluation-only L1 call runs it without the stores, the same sums in the same order: the same loss bits.
// LCGS_DEPTH_ALIGN_GIVEN computes no statistics: pass 1 only COUNTS the valid pixels (it reads the prior and the mask; g_v
// = weight / N_c sign(res) needs N_c in front of the pixel pass), one finish puts the caller's (s, t) into rec[0], then pass 5.
// The image's sums are finished by one workgroup (sum_partials_in_order); a patch has at most 32 tiles, which one thread adds
// in index order.  All algebra binary64, uncontracted; wave sums are the butterfly of ordered_sum.hpp, a workgroup's four wave
// sums are added as (0 + 1) + (2 + 3); no atomics: the same inputs give the same bits.
// Memory: the three statistics reads of depth, alpha, prior (and mask) are ordinary loads -- 1080p planes are 8.3 MB each and
// the next pass reads them again out of the L2 / MALL; the pixel pass is their last use and the gradients are written once
// for another kernel much later, so it loads all four inputs and stores with the streaming accesses of stream_access.hpp (the mask's
// bytes with the same builtin).  A wave reads two
// rows of 32 consecutive floats; rows start at any pixel (the grid's anchor and W are free), so the loads are single dwords.
#include "lcgs_hip.h" // LCGS_DEPTH_PRIOR_PEARSON, LCGS_DEPTH_PRIOR_L1

#include "launch.hpp"
#include "ordered_sum.hpp"
#include "stream_access.hpp"

namespace lcgs
{
namespace
{
constexpr int    kTW = kDepthPriorTileW, kTH = kDepthPriorTileH;
constexpr int    kThreads = kOrderedSumThreads;
constexpr double kEps = 1e-12;
static_assert(kTW * kTH == 2 * kThreads, "a thread owns two pixels of its tile");

// rec[group]: kDepthPriorRec doubles
enum { R_N = 0, R_MUV, R_MUM, R_AINV_N, R_B, R_S, R_T, R_COUNTED };
static_assert(R_COUNTED + 1 == kDepthPriorRec, "the record's size");

struct Pixel {
    double d, a, v, m;
    bool   valid;
};

// the workgroup's tile: its group, its slot, its first pixel (which may lie left of / above the image)
struct Tile {
    int     x0, y0, group;
    int64_t slot;
};
__device__ __forceinline__ Tile this_tile(const DepthPriorGrid& g)
{
    const int bx = blockIdx.x, by = blockIdx.y;
    const int gx = bx / g.gtx, gy = by / g.gty;
    Tile      t;
    t.x0    = bx * kTW - g.ox;
    t.y0    = by * kTH - g.oy;
    t.group = gy * g.groups_x + gx;
    t.slot  = (int64_t)t.group * (g.gtx * g.gty) + (by - gy * g.gty) * g.gtx + (bx - gx * g.gtx);
    return t;
}

// the validity of pixel o (in the image) and its prior; depth and alpha are not read.  STREAM: the pixel pass, the last use
template <bool STREAM>
__device__ __forceinline__ bool valid_prior(const float* __restrict__ prior, const uint8_t* __restrict__ mask, int64_t o, float& m)
{
    if (mask && (STREAM ? __builtin_nontemporal_load(mask + o) : mask[o]) == 0) return false;
    m = STREAM ? ld_stream(prior + o) : prior[o];
    return isfinite(m);
}

__device__ __forceinline__ double value_of(double d, double a, double alpha_min) { return d / (a < alpha_min ? alpha_min : a); }

// a workgroup's N sums: wave butterflies, then thread 0 adds the four wave sums as (0 + 1) + (2 + 3) -> out[0..N)
template <int N>
__device__ __forceinline__ void block_sums(double (&val)[N], double* __restrict__ out)
{
    __shared__ double s_red[N][kThreads / 64];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double s = wave_sum(val[k]);
        if ((threadIdx.x & 63) == 0) s_red[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = (s_red[k][0] + s_red[k][1]) + (s_red[k][2] + s_red[k][3]);
    }
}

// ---- pass 1
template <bool COUNT_ONLY>
__global__ void __launch_bounds__(kThreads) k_depth_prior_tile_sums(DepthPriorGrid g, double alpha_min, const float* __restrict__ depth,
                                                                    const float* __restrict__ alpha, const float* __restrict__ prior,
                                                                    const uint8_t* __restrict__ mask, double* __restrict__ tile1)
{
    const Tile t = this_tile(g);
    double     sum[3] = { 0.0, 0.0, 0.0 };
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int x = t.x0 + (threadIdx.x & 31), y = t.y0 + (threadIdx.x >> 5) + half * (kTH / 2);
        if (x < 0 || x >= g.W || y < 0 || y >= g.H) continue;
        const int64_t o = (int64_t)y * g.W + x;
        float         m;
        if (!valid_prior<false>(prior, mask, o, m)) continue;
        sum[0] += 1.0;
        if (!COUNT_ONLY) {
            sum[1] += value_of((double)depth[o], (double)alpha[o], alpha_min);
            sum[2] += (double)m;
        }
    }
    block_sums<3>(sum, tile1 + 3 * t.slot);
}

// ---- pass 2
__device__ __forceinline__ void write_means(const double (&s)[3], double* __restrict__ rec)
{
    const bool some = s[0] >= 1.0;
    rec[R_N]   = s[0];
    rec[R_MUV] = some ? s[1] / s[0] : 0.0;
    rec[R_MUM] = some ? s[2] / s[0] : 0.0;
}

__global__ void __launch_bounds__(kThreads) k_depth_prior_means_image(int64_t tiles, const double* __restrict__ tile1, double* __restrict__ rec)
{
    double s[3];
    if (sum_partials_in_order<3>(tiles, tile1, s)) write_means(s, rec);
}

// a patch's tiles (consecutive slots) in index order
__device__ __forceinline__ void sum_patch_tiles(const double* __restrict__ tile, int64_t group, int tpg, double (&s)[3])
{
    s[0] = s[1] = s[2] = 0.0;
    const double* p = tile + 3 * group * tpg;
    for (int i = 0; i < tpg; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += p[3 * i + k];
    }
}

__global__ void __launch_bounds__(kThreads) k_depth_prior_means_patch(int groups, int tpg, const double* __restrict__ tile1,
                                                                      double* __restrict__ rec)
{
    const int grp = blockIdx.x * kThreads + threadIdx.x;
    if (grp >= groups) return;
    double s[3];
    sum_patch_tiles(tile1, grp, tpg, s);
    write_means(s, rec + (int64_t)grp * kDepthPriorRec);
}

// ---- pass 3
__global__ void __launch_bounds__(kThreads) k_depth_prior_tile_centred(DepthPriorGrid g, double alpha_min, const float* __restrict__ depth,
                                                                       const float* __restrict__ alpha, const float* __restrict__ prior,
                                                                       const uint8_t* __restrict__ mask, const double* __restrict__ rec,
                                                                       double* __restrict__ tile2)
{
    const Tile    t = this_tile(g);
    const double* r = rec + (int64_t)t.group * kDepthPriorRec;
    double        sum[3] = { 0.0, 0.0, 0.0 };
    if (r[R_N] >= 2.0) { // (uniform over the workgroup)
        const double muv = r[R_MUV], mum = r[R_MUM];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int x = t.x0 + (threadIdx.x & 31), y = t.y0 + (threadIdx.x >> 5) + half * (kTH / 2);
            if (x < 0 || x >= g.W || y < 0 || y >= g.H) continue;
            const int64_t o = (int64_t)y * g.W + x;
            float         m;
            if (!valid_prior<false>(prior, mask, o, m)) continue;
            const double cv = value_of((double)depth[o], (double)alpha[o], alpha_min) - muv, cm = (double)m - mum;
            sum[0] += cv * cv;
            sum[1] += cm * cm;
            sum[2] += cv * cm;
        }
    }
    block_sums<3>(sum, tile2 + 3 * t.slot);
}

// ---- pass 4: a group's coefficients from its centred sums; gs = what the group adds to { G, N_c, sum (1 - r) }
__device__ __forceinline__ void write_coefficients(const double (&c)[3], double* __restrict__ rec, double (&gs)[3])
{
    const double n = rec[R_N];
    const bool   counted = n >= 2.0;
    double       ainv_n = 0.0, b = 0.0, s = 0.0, t = 0.0, r = 0.0;
    if (counted) {
        const double var_v = c[0] / n, var_m = c[1] / n, cov = c[2] / n;
        const double root = sqrt((var_v + kEps) * (var_m + kEps));
        r      = cov / root;
        ainv_n = 1.0 / (root * n);
        b      = cov / (var_v + kEps);
        s      = cov / (var_m + kEps);
        t      = rec[R_MUV] - s * rec[R_MUM];
    }
    rec[R_AINV_N]  = ainv_n;
    rec[R_B]       = b;
    rec[R_S]       = s;
    rec[R_T]       = t;
    rec[R_COUNTED] = counted ? 1.0 : 0.0;
    gs[0] = counted ? 1.0 : 0.0;
    gs[1] = counted ? n : 0.0;
    gs[2] = counted ? 1.0 - r : 0.0;
}

// hdr = { G, N_c }; the Pearson loss; d_stats = { N_c, G, s, t }
__device__ __forceinline__ void write_header(const double (&gs)[3], int kind, double weight, double s, double t, double* __restrict__ hdr,
                                             float* __restrict__ loss, float* __restrict__ stats)
{
    hdr[0] = gs[0];
    hdr[1] = gs[1];
    if (kind == LCGS_DEPTH_PRIOR_PEARSON) loss[0] = gs[0] > 0.0 ? (float)(weight / gs[0] * gs[2]) : 0.0f;
    if (stats) {
        stats[0] = (float)gs[1];
        stats[1] = (float)gs[0];
        stats[2] = (float)s;
        stats[3] = (float)t;
    }
}

__global__ void __launch_bounds__(kThreads) k_depth_prior_coefficients_image(int64_t tiles, const double* __restrict__ tile2, int kind,
                                                                             double weight, double* __restrict__ rec, double* __restrict__ hdr,
                                                                             float* __restrict__ loss, float* __restrict__ stats)
{
    double c[3], gs[3];
    if (!sum_partials_in_order<3>(tiles, tile2, c)) return;
    write_coefficients(c, rec, gs);
    write_header(gs, kind, weight, rec[R_S], rec[R_T], hdr, loss, stats);
}

__global__ void __launch_bounds__(kThreads) k_depth_prior_coefficients_patch(int groups, int tpg, const double* __restrict__ tile2,
                                                                             double* __restrict__ rec, double* __restrict__ gsum)
{
    const int grp = blockIdx.x * kThreads + threadIdx.x;
    if (grp >= groups) return;
    double c[3], gs[3];
    sum_patch_tiles(tile2, grp, tpg, c);
    write_coefficients(c, rec + (int64_t)grp * kDepthPriorRec, gs);
#pragma unroll
    for (int k = 0; k < 3; ++k) gsum[3 * (int64_t)grp + k] = gs[k];
}

__global__ void __launch_bounds__(kThreads) k_depth_prior_groups_finish(int64_t groups, const double* __restrict__ gsum, int kind, double weight,
                                                                        double* __restrict__ hdr, float* __restrict__ loss,
                                                                        float* __restrict__ stats)
{
    double gs[3];
    if (sum_partials_in_order<3>(groups, gsum, gs)) write_header(gs, kind, weight, 0.0, 0.0, hdr, loss, stats);
}

// LCGS_DEPTH_ALIGN_GIVEN: the counts of pass 1 -> N_c; the one group is counted from 1 valid pixel on and carries the caller's pair
__global__ void __launch_bounds__(kThreads) k_depth_prior_given_finish(int64_t tiles, const double* __restrict__ tile1, double s, double t,
                                                                       double* __restrict__ rec, double* __restrict__ hdr,
                                                                       float* __restrict__ stats)
{
    double c[3];
    if (!sum_partials_in_order<3>(tiles, tile1, c)) return;
    const bool counted = c[0] >= 1.0;
    rec[R_N]       = c[0];
    rec[R_S]       = s;
    rec[R_T]       = t;
    rec[R_COUNTED] = counted ? 1.0 : 0.0;
    const double gs[3] = { counted ? 1.0 : 0.0, c[0], 0.0 };
    write_header(gs, LCGS_DEPTH_PRIOR_L1, 0.0, s, t, hdr, nullptr, stats);
}

// ---- pass 5
template <int KIND, bool GRAD>
__global__ void __launch_bounds__(kThreads) k_depth_prior_pixels(DepthPriorGrid g, double alpha_min, double weight, const float* __restrict__ depth,
                                                                 const float* __restrict__ alpha, const float* __restrict__ prior,
                                                                 const uint8_t* __restrict__ mask, const double* __restrict__ rec,
                                                                 const double* __restrict__ hdr, float* __restrict__ dL_ddepth,
                                                                 float* __restrict__ dL_dalpha, double* __restrict__ l1_part)
{
    const Tile    t = this_tile(g);
    const double* r = rec + (int64_t)t.group * kDepthPriorRec;
    const bool    counted = r[R_COUNTED] != 0.0;
    // Pearson: g_v = k (cm - B cv), k = -weight / (G n sqrt(..)); L1: g_v = k sign(res), k = weight / N_c
    const double  total = hdr[KIND == LCGS_DEPTH_PRIOR_PEARSON ? 0 : 1];
    const double  per   = total > 0.0 ? weight / total : 0.0;
    const double  k = KIND == LCGS_DEPTH_PRIOR_PEARSON ? -per * r[R_AINV_N] : per;
    const double  muv = r[R_MUV], mum = r[R_MUM], B = r[R_B], s = r[R_S], sh = r[R_T];
    double        sum[1] = { 0.0 };
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int x = t.x0 + (threadIdx.x & 31), y = t.y0 + (threadIdx.x >> 5) + half * (kTH / 2);
        if (x < 0 || x >= g.W || y < 0 || y >= g.H) continue;
        const int64_t o = (int64_t)y * g.W + x;
        float         mf = 0.0f;
        double        gd = 0.0, ga = 0.0;
        if (counted && valid_prior<true>(prior, mask, o, mf)) {
            const double d = (double)ld_stream(depth + o), a = (double)ld_stream(alpha + o), m = (double)mf;
            const double v = value_of(d, a, alpha_min);
            double       gv;
            if (KIND == LCGS_DEPTH_PRIOR_PEARSON) {
                gv = k * ((m - mum) - B * (v - muv));
            } else {
                const double res = v - (s * m + sh);
                sum[0] += fabs(res);
                gv = k * (double)((res > 0.0) - (res < 0.0)); // sign(0) = 0
            }
            gd = gv / (a < alpha_min ? alpha_min : a);
            if (a >= alpha_min) ga = -gv * d / (a * a); // (the clamp passes its gradient at equality)
        }
        if (GRAD) {
            st_stream(dL_ddepth + o, (float)gd);
            st_stream(dL_dalpha + o, (float)ga);
        }
    }
    if (KIND == LCGS_DEPTH_PRIOR_L1) block_sums<1>(sum, l1_part + t.slot);
}

__global__ void __launch_bounds__(kThreads) k_depth_prior_l1_finish(int64_t tiles, const double* __restrict__ l1_part, const double* __restrict__ hdr,
                                                                    double weight, float* __restrict__ loss)
{
    double sum[1];
    if (sum_partials_in_order<1>(tiles, l1_part, sum)) loss[0] = hdr[1] > 0.0 ? (float)(weight / hdr[1] * sum[0]) : 0.0f;
}
} // namespace

DepthPriorGrid depth_prior_grid(int W, int H, int patch, int patch_x, int patch_y)
{
    DepthPriorGrid g;
    g.W  = W;
    g.H  = H;
    g.ox = patch ? patch_x : 0;
    g.oy = patch ? patch_y : 0;
    const int tiles_x = (W + g.ox + kTW - 1) / kTW, tiles_y = (H + g.oy + kTH - 1) / kTH;
    g.gtx      = patch ? patch / kTW : tiles_x;
    g.gty      = patch ? patch / kTH : tiles_y;
    g.groups_x = (tiles_x + g.gtx - 1) / g.gtx;
    g.groups_y = (tiles_y + g.gty - 1) / g.gty;
    return g;
}

DepthPriorWorkspace depth_prior_workspace(const DepthPriorGrid& g, double* base)
{
    const size_t        tiles = (size_t)depth_prior_tiles(g), groups = (size_t)depth_prior_groups(g);
    const size_t        rec = 8, gsum = rec + kDepthPriorRec * groups, tile1 = gsum + 3 * groups, tile2 = tile1 + 3 * tiles,
                        l1_part = tile2 + 3 * tiles;
    DepthPriorWorkspace w = {};
    w.doubles = l1_part + tiles;
    if (base) w = { base, base + rec, base + gsum, base + tile1, base + tile2, base + l1_part, w.doubles };
    return w;
}

void launch_depth_prior(const DepthPriorGrid& g, const DepthPriorTerm& term, const float* depth, const float* alpha, const float* prior,
                        const uint8_t* mask, float* dL_ddepth, float* dL_dalpha, float* loss, float* stats, const DepthPriorWorkspace& w,
                        hipStream_t stream)
{
    // every tile of every group is launched, the ones of a border patch that lie outside the image too: they read nothing and
    // write zeros into their slots
    const dim3    grid((unsigned)(g.groups_x * g.gtx), (unsigned)(g.groups_y * g.gty)), block(kThreads);
    const int64_t tiles = depth_prior_tiles(g);
    const int     groups = (int)depth_prior_groups(g), tpg = g.gtx * g.gty;
    const dim3    group_grid((unsigned)((groups + kThreads - 1) / kThreads));
    // the image's sums are finished by one workgroup and report the fit; a patch grid goes the per-patch way even where it
    // has a single group on this image (a small frame, some offsets of a jittered grid): the same path and no fit in d_stats
    // at every offset
    const bool    whole = !term.patch, grad = dL_ddepth != nullptr;
    const double  alpha_min = term.alpha_min, weight = term.weight;
    if (term.given) {
        hipLaunchKernelGGL(k_depth_prior_tile_sums<true>, grid, block, 0, stream, g, alpha_min, depth, alpha, prior, mask, w.tile1);
        hipLaunchKernelGGL(k_depth_prior_given_finish, dim3(1), block, 0, stream, tiles, w.tile1, term.scale, term.shift, w.rec, w.hdr, stats);
    } else {
        hipLaunchKernelGGL(k_depth_prior_tile_sums<false>, grid, block, 0, stream, g, alpha_min, depth, alpha, prior, mask, w.tile1);
        if (whole)
            hipLaunchKernelGGL(k_depth_prior_means_image, dim3(1), block, 0, stream, tiles, w.tile1, w.rec);
        else
            hipLaunchKernelGGL(k_depth_prior_means_patch, group_grid, block, 0, stream, groups, tpg, w.tile1, w.rec);
        hipLaunchKernelGGL(k_depth_prior_tile_centred, grid, block, 0, stream, g, alpha_min, depth, alpha, prior, mask, w.rec, w.tile2);
        if (whole) {
            hipLaunchKernelGGL(k_depth_prior_coefficients_image, dim3(1), block, 0, stream, tiles, w.tile2, term.kind, weight, w.rec, w.hdr, loss,
                               stats);
        } else {
            hipLaunchKernelGGL(k_depth_prior_coefficients_patch, group_grid, block, 0, stream, groups, tpg, w.tile2, w.rec, w.gsum);
            hipLaunchKernelGGL(k_depth_prior_groups_finish, dim3(1), block, 0, stream, (int64_t)groups, w.gsum, term.kind, weight, w.hdr, loss,
                               stats);
        }
    }
    if (term.kind == LCGS_DEPTH_PRIOR_PEARSON) {
        if (grad)
            hipLaunchKernelGGL((k_depth_prior_pixels<LCGS_DEPTH_PRIOR_PEARSON, true>), grid, block, 0, stream, g, alpha_min, weight, depth, alpha,
                               prior, mask, w.rec, w.hdr, dL_ddepth, dL_dalpha, w.l1_part);
        return;
    }
    if (grad)
        hipLaunchKernelGGL((k_depth_prior_pixels<LCGS_DEPTH_PRIOR_L1, true>), grid, block, 0, stream, g, alpha_min, weight, depth, alpha, prior,
                           mask, w.rec, w.hdr, dL_ddepth, dL_dalpha, w.l1_part);
    else
        hipLaunchKernelGGL((k_depth_prior_pixels<LCGS_DEPTH_PRIOR_L1, false>), grid, block, 0, stream, g, alpha_min, weight, depth, alpha, prior,
                           mask, w.rec, w.hdr, dL_ddepth, dL_dalpha, w.l1_part);
    hipLaunchKernelGGL(k_depth_prior_l1_finish, dim3(1), block, 0, stream, tiles, w.l1_part, w.hdr, weight, loss);
}

} // namespace lcgs

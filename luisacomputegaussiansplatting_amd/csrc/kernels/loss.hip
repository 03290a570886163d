// loss.hip -- the 3DGS photometric loss (1 - lambda) mean|x - y| + lambda (1 - SSIM(x, y)) and its gradient with respect to x
// (the definition is the contract in include/lcgs_hip.h).  No reference counterpart (doc/roadmap.md:4 only
// names training).  Two passes over 32 x 16 output tiles of one channel, one 256-thread workgroup each, both a separable
// 11-tap convolution staged through LDS (a row pass into LDS planes, a column pass into registers):
//   pass A  x, y (tile + 5-pixel halo, zeros outside the image) -> the five statistics -> ssim and its three partial
//           derivatives a, b, c per pixel (stored for pass B) + one { sum ssim, sum |x - y| } pair per workgroup
//   pass B  a, b, c (tile + halo, zeros outside the image: the window is symmetric, so the adjoint of the zero-padded
//           convolution is the same convolution) -> G*a + 2 x G*b + y G*c -> dL/dx with the L1 term, written once
//   finish  one workgroup sums the pairs in index order -> loss, { L1, SSIM }
// Nothing is accumulated with atomics: the same inputs give the same bits.
// Precision: sigma^2 = G*x^2 - mu^2 cancels in the flat regions rendered frames are made of (both terms ~ x^2, the
// difference is compared with C2 = 9e-4), so pass A carries its planes, statistics and the ssim algebra in binary64 (x^2 and
// x y are then exact) and rounds a, b, c once; every sum over pixels is binary64 too.  Pass B has no such difference of
// squares: binary32 planes, binary64 column accumulators and final expression, one rounding of the result.
// LDS pitches (64 banks of 4 bytes; a wave is two tile rows of 32 columns):
//   row-filtered planes: pitch 32 elements.  binary32 (pass B): the two rows of a wave are 32 words apart, so its 64 lanes
//   read 64 consecutive words, one per bank.  binary64 (pass A): a 64-bit read is served 32 lanes at a time, and the 32
//   lanes of one row read 64 consecutive words.  Either way the column pass, which walks the same column down consecutive
//   rows, is conflict free.
//   staged inputs: the planes of one row sit side by side at a 48-word spacing (42 used) and the row pitch is 32 mod 64 words
//   (96 for x | y, 160 for a | b | c), so the row pass is conflict free for the same reason.
// Below it, on the same tiles and the same finish step: the normal-consistency loss of a frame's depth, alpha and normal maps
// and its three gradients in one kernel (k_normal_consistency; its comment has the phases and the LDS reasoning).
#include "launch.hpp"
#include "ordered_sum.hpp"
#include "stream_access.hpp"

namespace lcgs
{
namespace
{
constexpr int kR = 5, kTaps = 2 * kR + 1; // the 11 x 11 window
constexpr int kTW = 32, kTH = 16;         // outputs of a workgroup
constexpr int kInW = kTW + 2 * kR, kInH = kTH + 2 * kR; // ... and what they read: 42 x 26
constexpr int kSlot = 48;                 // spacing of the planes inside a staged row
constexpr int kPitchA = 96, kPitchB = 160;
constexpr int kThreads = kOrderedSumThreads;
static_assert(kInW <= kSlot && kSlot + kInW <= kPitchA && 2 * kSlot + kInW <= kPitchB, "staged planes overlap");
static_assert(kPitchA % 64 == 32 && kPitchB % 64 == 32, "row pitch must be 32 mod 64 banks");

// w[k] = exp(-(k - 5)^2 / (2 1.5^2)) / sum, the binary64 values rounded to binary32
__device__ const float kGauss[kTaps] = { 0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                                         0x1.b43c4p-3f,   0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f };
constexpr double kC1 = 0.01 * 0.01, kC2 = 0.03 * 0.03;

// ---- pass A
template <bool STORE>
__global__ void __launch_bounds__(kThreads) k_photometric_stats(int W, int H, const float* __restrict__ img,
                                                                const float* __restrict__ target, float* __restrict__ abc,
                                                                double* __restrict__ partials)
{
    __shared__ float  s_in[kInH][kPitchA];  // x at [0, 42), y at [48, 90)
    __shared__ double s_row[5][kInH][kTW];  // row-filtered x, y, x^2, y^2, x y
    __shared__ double s_red[2][kThreads / 64];
    const int     tid = threadIdx.x;
    const int     x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int64_t plane = (int64_t)W * H, chan = (int64_t)blockIdx.z * plane;
    for (int i = tid; i < kInH * kInW; i += kThreads) {
        const int  r = i / kInW, c = i - r * kInW;
        const int  gy = y0 - kR + r, gx = x0 - kR + c;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const int64_t o = chan + (int64_t)gy * W + gx;
        s_in[r][c]         = in ? img[o] : 0.0f;
        s_in[r][kSlot + c] = in ? target[o] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kInH * kTW; i += kThreads) {
        const int r = i >> 5, c = i & 31;
        double    sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const double w = (double)kGauss[k], xv = (double)s_in[r][c + k], yv = (double)s_in[r][kSlot + c + k];
            sx  = fma(w, xv, sx);
            sy  = fma(w, yv, sy);
            sxx = fma(w, xv * xv, sxx);
            syy = fma(w, yv * yv, syy);
            sxy = fma(w, xv * yv, sxy);
        }
        s_row[0][r][c] = sx;
        s_row[1][r][c] = sy;
        s_row[2][r][c] = sxx;
        s_row[3][r][c] = syy;
        s_row[4][r][c] = sxy;
    }
    __syncthreads();
    double sum_ssim = 0.0, sum_l1 = 0.0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int r = (tid >> 5) + half * (kTH / 2), c = tid & 31;
        double    m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const double w = (double)kGauss[k];
            m1  = fma(w, s_row[0][r + k][c], m1);
            m2  = fma(w, s_row[1][r + k][c], m2);
            e11 = fma(w, s_row[2][r + k][c], e11);
            e22 = fma(w, s_row[3][r + k][c], e22);
            e12 = fma(w, s_row[4][r + k][c], e12);
        }
        const int gx = x0 + c, gy = y0 + r;
        if (gx < W && gy < H) {
            const double s11 = e11 - m1 * m1, s22 = e22 - m2 * m2, s12 = e12 - m1 * m2;
            const double A1 = 2.0 * m1 * m2 + kC1, A2 = 2.0 * s12 + kC2;
            const double B1 = m1 * m1 + m2 * m2 + kC1, B2 = s11 + s22 + kC2;
            const double inv = 1.0 / (B1 * B2), ssim = A1 * A2 * inv;
            sum_ssim += ssim;
            sum_l1 += fabs((double)s_in[r + kR][c + kR] - (double)s_in[r + kR][kSlot + c + kR]);
            if (STORE) {
                // b = d ssim / d sigma1^2, c = d / d sigma12; a = d / d mu1 with sigma1^2 = G*x^2 - mu1^2 and
                // sigma12 = G*xy - mu1 mu2 expanded: the partial at fixed sigmas, - 2 mu1 b - mu2 c
                const double    db = -ssim / B2, dc = 2.0 * A1 * inv;
                const double    da = 2.0 * (m2 * A2 * inv - m1 * ssim / B1) - 2.0 * m1 * db - m2 * dc;
                const int64_t   o  = chan + (int64_t)gy * W + gx;
                const int64_t   n  = 3 * plane;
                abc[o]         = (float)da;
                abc[n + o]     = (float)db;
                abc[2 * n + o] = (float)dc;
            }
        }
    }
    sum_ssim = wave_sum(sum_ssim);
    sum_l1   = wave_sum(sum_l1);
    if ((tid & 63) == 0) {
        s_red[0][tid >> 6] = sum_ssim;
        s_red[1][tid >> 6] = sum_l1;
    }
    __syncthreads();
    if (tid == 0) {
        const int64_t wg = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partials[2 * wg + 0] = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
        partials[2 * wg + 1] = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
    }
}

// ---- pass B
__global__ void __launch_bounds__(kThreads) k_photometric_grad(int W, int H, const float* __restrict__ img,
                                                               const float* __restrict__ target, const float* __restrict__ abc,
                                                               float lambda, float* __restrict__ dL)
{
    __shared__ float s_in[kInH][kPitchB];  // a at [0, 42), b at [48, 90), c at [96, 138)
    __shared__ float s_row[3][kInH][kTW];
    const int     tid = threadIdx.x;
    const int     x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int64_t plane = (int64_t)W * H, chan = (int64_t)blockIdx.z * plane, n = 3 * plane;
    const double  l1_scale = (1.0 - (double)lambda) / (double)n, ssim_scale = (double)lambda / (double)n;
    if (lambda == 0.0f) { // the L1 term alone: the workspace is not read (it may hold anything)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int gx = x0 + (tid & 31), gy = y0 + (tid >> 5) + half * (kTH / 2);
            if (gx < W && gy < H) {
                const int64_t o = chan + (int64_t)gy * W + gx;
                const float   xv = ld_stream(img + o), yv = ld_stream(target + o);
                dL[o] = (float)(l1_scale * (double)((xv > yv) - (xv < yv)));
            }
        }
        return;
    }
    for (int i = tid; i < kInH * kInW; i += kThreads) {
        const int  r = i / kInW, c = i - r * kInW;
        const int  gy = y0 - kR + r, gx = x0 - kR + c;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const int64_t o = chan + (int64_t)gy * W + gx;
        s_in[r][c]             = in ? abc[o] : 0.0f;
        s_in[r][kSlot + c]     = in ? abc[n + o] : 0.0f;
        s_in[r][2 * kSlot + c] = in ? abc[2 * n + o] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kInH * kTW; i += kThreads) {
        const int r = i >> 5, c = i & 31;
        float     sa = 0.0f, sb = 0.0f, sc = 0.0f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const float w = kGauss[k];
            sa = fmaf(w, s_in[r][c + k], sa);
            sb = fmaf(w, s_in[r][kSlot + c + k], sb);
            sc = fmaf(w, s_in[r][2 * kSlot + c + k], sc);
        }
        s_row[0][r][c] = sa;
        s_row[1][r][c] = sb;
        s_row[2][r][c] = sc;
    }
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int r = (tid >> 5) + half * (kTH / 2), c = tid & 31;
        const int gx = x0 + c, gy = y0 + r;
        if (gx >= W || gy >= H) continue;
        double ga = 0.0, gb = 0.0, gc = 0.0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const double w = (double)kGauss[k];
            ga = fma(w, (double)s_row[0][r + k][c], ga);
            gb = fma(w, (double)s_row[1][r + k][c], gb);
            gc = fma(w, (double)s_row[2][r + k][c], gc);
        }
        const int64_t o  = chan + (int64_t)gy * W + gx;
        const float   xv = ld_stream(img + o), yv = ld_stream(target + o);
        const double  sgn = (double)((xv > yv) - (xv < yv)); // sign(0) = 0
        dL[o] = (float)(l1_scale * sgn - ssim_scale * (ga + 2.0 * (double)xv * gb + (double)yv * gc));
    }
}

// ---- finish: the workgroups' partials in index order (ordered_sum.hpp)
__global__ void __launch_bounds__(kThreads) k_photometric_finish(int64_t num, double n, const double* __restrict__ partials,
                                                                 float lambda, float* __restrict__ loss, float* __restrict__ terms)
{
    double sums[2];
    if (!sum_partials_in_order<2>(num, partials, sums)) return;
    const double ssim = sums[0] / n, l1 = sums[1] / n, lam = (double)lambda;
    loss[0] = (float)((1.0 - lam) * l1 + lam * (1.0 - ssim));
    if (terms) {
        terms[0] = (float)l1;
        terms[1] = (float)ssim;
    }
}

// ---- the normal-consistency loss (the contract in include/lcgs_hip.h): one workgroup per 32 x 16 tile, three phases
//   stage   z = depth / max(alpha, alpha_min) of the tile + a 2-pixel halo (0 outside the image: only cells that are not interior
//           would read it, and those read nothing) and the ray slopes rx, ry of its columns and rows -> LDS
//   cells   every cell of the tile + a 1-pixel halo (34 x 18, a flat index over the threads): ex, ey, m, s, nt from the staged z,
//           the rendered normal from global memory -> g_ex, g_ey (0 for a cell that is not interior) into LDS, six planes;
//           a cell of the tile proper also adds its term to the thread's sum and writes dL/dnormal
//   gather  every pixel of the tile: G from its four neighbours' cells, g_z -> dL/ddepth, dL/dalpha, written once
// All binary64, uncontracted; each output rounded once.  The evaluation-only kernel runs stage and the tile's own cells in the
// same order with the same operations, so its partial is the gradient kernel's bit for bit.
// LDS (34.5 KB: four workgroups a CU): every array holds doubles at consecutive indices for consecutive lanes.  The gather
// reads four cells of a plane per pixel, and the 32 lanes that one ds_read_b64 serves together are one tile row: 32 consecutive
// doubles = the 64 banks once each, whatever the pitch (34).  The cell phase writes plane[i] for lane i (ds_write_b64 serves 16
// lanes together: 32 consecutive words, the 32 banks once each) and reads z at (row, column) of a flat cell index: 32
// consecutive cells span at most two rows of pitch 36, i.e. 32 of 34 consecutive doubles with a hole of two -- at most two
// 2-way conflicts per read, on five reads a cell beside some 150 binary64 operations.
// The planes were measured against every pixel recomputing its own and its four neighbours' cells (no planes, 6 KB of LDS, twice
// the waves a SIMD): 47.7 us against 63.7 us at 1920 x 1080 (profiles/normal_consistency_bench.txt), so the planes stay.
constexpr int kZW = kTW + 4, kZH = kTH + 4; // staged z: 36 x 20
constexpr int kGW = kTW + 2, kGH = kTH + 2; // cells: 34 x 18

template <bool GRAD>
__global__ void __launch_bounds__(kThreads) k_normal_consistency(int W, int H, double tanx, double tany, double scale,
                                                                 double alpha_min, const float* __restrict__ depth,
                                                                 const float* __restrict__ alpha, const float* __restrict__ normal,
                                                                 float* __restrict__ dL_ddepth, float* __restrict__ dL_dalpha,
                                                                 float* __restrict__ dL_dnormal, double* __restrict__ partials)
{
    __shared__ double s_z[kZH][kZW];
    __shared__ double s_rx[kZW], s_ry[kZH];
    __shared__ double s_g[6][GRAD ? kGH * kGW : 1]; // g_ex at planes 0..2, g_ey at 3..5
    __shared__ double s_red[kThreads / 64];
    const int     tid = threadIdx.x;
    const int     x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int64_t plane = (int64_t)W * H;
    for (int i = tid; i < kZH * kZW; i += kThreads) {
        const int  r = i / kZW, c = i - r * kZW;
        const int  gy = y0 - 2 + r, gx = x0 - 2 + c;
        double     z = 0.0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const int64_t o = (int64_t)gy * W + gx;
            const double  a = (double)alpha[o];
            z = (double)depth[o] / (a < alpha_min ? alpha_min : a);
        }
        s_z[r][c] = z;
    }
    if (tid < kZW) s_rx[tid] = (((double)(x0 - 2 + tid) + 0.5) / (double)W * 2.0 - 1.0) * tanx;
    if (tid >= 64 && tid < 64 + kZH) s_ry[tid - 64] = (((double)(y0 - 2 + tid - 64) + 0.5) / (double)H * 2.0 - 1.0) * tany;
    __syncthreads();
    double sum = 0.0;
    for (int i = tid; i < kGH * kGW; i += kThreads) {
        const int  r = i / kGW, c = i - r * kGW; // cell (r, c) is pixel (x0 - 1 + c, y0 - 1 + r): z at s_z[r + 1][c + 1]
        const int  gy = y0 - 1 + r, gx = x0 - 1 + c;
        const bool own = r >= 1 && r <= kTH && c >= 1 && c <= kTW; // a cell of the tile proper
        if (!GRAD && !own) continue;
        const int64_t o = (int64_t)gy * W + gx;
        if (gx >= 1 && gx <= W - 2 && gy >= 1 && gy <= H - 2) { // interior: its four neighbours are pixels
            const double zxm = s_z[r + 1][c], zxp = s_z[r + 1][c + 2], zym = s_z[r][c + 1], zyp = s_z[r + 2][c + 1];
            const double rxm = s_rx[c], rx = s_rx[c + 1], rxp = s_rx[c + 2], rym = s_ry[r], ry = s_ry[r + 1], ryp = s_ry[r + 2];
            const double ex0 = rxp * zxp - rxm * zxm, ex1 = ry * zxp - ry * zxm, ex2 = zxp - zxm;
            const double ey0 = rx * zyp - rx * zym, ey1 = ryp * zyp - rym * zym, ey2 = zyp - zym;
            const double m0 = ey1 * ex2 - ey2 * ex1, m1 = ey2 * ex0 - ey0 * ex2, m2 = ey0 * ex1 - ey1 * ex0; // ey x ex
            const double inv = 1.0 / sqrt((m0 * m0 + m1 * m1 + m2 * m2) + 1e-20);
            const double nt0 = m0 * inv, nt1 = m1 * inv, nt2 = m2 * inv;
            const double n0 = (double)normal[o], n1 = (double)normal[plane + o], n2 = (double)normal[2 * plane + o];
            if (own) sum += (double)alpha[o] - (n0 * nt0 + n1 * nt1 + n2 * nt2);
            if (GRAD) {
                if (own) {
                    dL_dnormal[o]             = (float)(-scale * nt0);
                    dL_dnormal[plane + o]     = (float)(-scale * nt1);
                    dL_dnormal[2 * plane + o] = (float)(-scale * nt2);
                }
                // g_m = -c (n / s - m (m . n) / s^3), g_ey = ex x g_m, g_ex = g_m x ey
                const double t   = (m0 * n0 + m1 * n1 + m2 * n2) * (inv * inv * inv);
                const double gm0 = -scale * (n0 * inv - m0 * t), gm1 = -scale * (n1 * inv - m1 * t), gm2 = -scale * (n2 * inv - m2 * t);
                s_g[0][i] = gm1 * ey2 - gm2 * ey1;
                s_g[1][i] = gm2 * ey0 - gm0 * ey2;
                s_g[2][i] = gm0 * ey1 - gm1 * ey0;
                s_g[3][i] = ex1 * gm2 - ex2 * gm1;
                s_g[4][i] = ex2 * gm0 - ex0 * gm2;
                s_g[5][i] = ex0 * gm1 - ex1 * gm0;
            }
        } else if (GRAD) {
#pragma unroll
            for (int k = 0; k < 6; ++k) s_g[k][i] = 0.0;
            if (own && gx < W && gy < H) { // a border pixel (an own cell has gx, gy >= 0)
                dL_dnormal[o]             = 0.0f;
                dL_dnormal[plane + o]     = 0.0f;
                dL_dnormal[2 * plane + o] = 0.0f;
            }
        }
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    __syncthreads(); // (the planes of s_g too)
    if (tid == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    if (!GRAD) return;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int r = (tid >> 5) + half * (kTH / 2), c = tid & 31;
        const int gx = x0 + c, gy = y0 + r;
        if (gx >= W || gy >= H) continue;
        const int i = (r + 1) * kGW + (c + 1); // the pixel's own cell
        // G = g_ex(q - x^) - g_ex(q + x^) + g_ey(q - y^) - g_ey(q + y^)
        const double G0 = ((s_g[0][i - 1] - s_g[0][i + 1]) + s_g[3][i - kGW]) - s_g[3][i + kGW];
        const double G1 = ((s_g[1][i - 1] - s_g[1][i + 1]) + s_g[4][i - kGW]) - s_g[4][i + kGW];
        const double G2 = ((s_g[2][i - 1] - s_g[2][i + 1]) + s_g[5][i - kGW]) - s_g[5][i + kGW];
        const double gz = (G0 * s_rx[c + 2] + G1 * s_ry[r + 2]) + G2;
        const int64_t o = (int64_t)gy * W + gx;
        const double  a = (double)alpha[o], d = (double)depth[o];
        double        ga = gx >= 1 && gx <= W - 2 && gy >= 1 && gy <= H - 2 ? scale : 0.0;
        if (a >= alpha_min) ga += -gz * d / (a * a); // (the clamp passes its gradient at equality)
        st_stream(dL_ddepth + o, (float)(gz / (a < alpha_min ? alpha_min : a)));
        st_stream(dL_dalpha + o, (float)ga);
    }
}

__global__ void __launch_bounds__(kThreads) k_normal_consistency_finish(int64_t num, double scale, const double* __restrict__ partials,
                                                                        float* __restrict__ loss)
{
    double sum[1];
    if (sum_partials_in_order<1>(num, partials, sum)) loss[0] = (float)(scale * sum[0]);
}

inline dim3 tile_grid(int W, int H) { return dim3((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH), 3u); }
} // namespace

int64_t normal_consistency_workgroups(int W, int H) { return (int64_t)((W + kTW - 1) / kTW) * ((H + kTH - 1) / kTH); }

void launch_normal_consistency(int W, int H, double tanx, double tany, double scale, double alpha_min, const float* depth,
                               const float* alpha, const float* normal, float* dL_ddepth, float* dL_dalpha, float* dL_dnormal,
                               double* partials, float* loss, hipStream_t stream)
{
    const dim3 grid((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH));
    if (dL_ddepth)
        hipLaunchKernelGGL(k_normal_consistency<true>, grid, dim3(kThreads), 0, stream, W, H, tanx, tany, scale, alpha_min, depth,
                           alpha, normal, dL_ddepth, dL_dalpha, dL_dnormal, partials);
    else
        hipLaunchKernelGGL(k_normal_consistency<false>, grid, dim3(kThreads), 0, stream, W, H, tanx, tany, scale, alpha_min, depth,
                           alpha, normal, dL_ddepth, dL_dalpha, dL_dnormal, partials);
    hipLaunchKernelGGL(k_normal_consistency_finish, dim3(1), dim3(kThreads), 0, stream, normal_consistency_workgroups(W, H), scale,
                       partials, loss);
}

int64_t photometric_workgroups(int W, int H)
{
    const dim3 g = tile_grid(W, H);
    return (int64_t)g.x * g.y * g.z;
}

void launch_photometric_stats(int W, int H, const float* img, const float* target, float* abc, double* partials,
                              hipStream_t stream)
{
    if (abc)
        hipLaunchKernelGGL(k_photometric_stats<true>, tile_grid(W, H), dim3(kThreads), 0, stream, W, H, img, target, abc, partials);
    else
        hipLaunchKernelGGL(k_photometric_stats<false>, tile_grid(W, H), dim3(kThreads), 0, stream, W, H, img, target, abc, partials);
}

void launch_photometric_grad(int W, int H, const float* img, const float* target, const float* abc, float lambda, float* dL,
                             hipStream_t stream)
{
    hipLaunchKernelGGL(k_photometric_grad, tile_grid(W, H), dim3(kThreads), 0, stream, W, H, img, target, abc, lambda, dL);
}

void launch_photometric_finish(int W, int H, const double* partials, float lambda, float* loss, float* terms,
                               hipStream_t stream)
{
    hipLaunchKernelGGL(k_photometric_finish, dim3(1), dim3(kThreads), 0, stream, photometric_workgroups(W, H),
                       3.0 * (double)W * (double)H, partials, lambda, loss, terms);
}

} // namespace lcgs

// splat_backward.hpp -- the per-splat backward as ONE set of device expressions: 2-D gradients -> the gradients of a splat's
// view-space position and projected covariance axes, and from there its parameters (geom_backward) or the camera
// (camera_grad.hip), and the colour step's view-direction part of dL/dpos.  backward.hip's preprocess kernels and
// camera_grad.hip call these with values in registers and keep their own loads and stores; the build does not contract
// (-ffp-contract=off), so one source expression gives the same bits in every caller (adam_rows.hpp is the precedent).
#pragma once

#include "launch.hpp"

namespace lcgs
{

// What geom_backward_t forms on its way and the parameter pass drops: the gradient w.r.t. the view-space position (dv: the
// covariance path through the frustum clamp + the pixel-mean path), w.r.t. the two projected covariance axes T0 / T1 (as
// independent variables), and the four entries of the projection Jacobian that scale the view rows inside T0 / T1.
template <typename FP>
struct GeomCameraTerms {
    FP dv[3], dT0[3], dT1[3], j00, j11, j02, j12;
};

// ---------------------------------------------------------------------------------------------------------------
// 2-D gradients -> parameter gradients, one lane per surviving splat.
// ---------------------------------------------------------------------------------------------------------------
// dL/d{pixel mean (gmx, gmy), conic (gA, gB, gC)} -> dL/d{pos (gp), scale (gs), rotq (gq: r,x,y,z)} through the EWA
// projection, in precision R.  The forward quantities are recomputed (the order of gs_math.hpp is irrelevant for the
// derivative).  cov_trace = a + c of the filtered 2-D covariance (>= its larger eigenvalue: the splat's footprint).
// aa_rho != NULL: a row of an antialiased frame (CamParams::raster_mode).  The frame blended with o' = opacity * rho,
// rho = sqrt(max(0, d0 / d1)), d0 = a0 c0 - b^2 of the raw and d1 = a c - b^2 of the filtered covariance (the unfloored d1, not
// D = d1 + 1e-6); aa_go = dL/do' * opacity.  rho is returned through aa_rho (dL/dopacity = dL/do' * rho is the caller's) and
// aa_go * drho/d(a, b, c) joins g00 / g01 / g11, so the parameter gradients and the camera terms carry it with no further code.
template <typename FP>
__device__ __forceinline__ void geom_backward_t(const CamParams& cp, FP scale_modifier, FP px, FP py, FP pz, FP sc0, FP sc1, FP sc2,
                                                FP qw_, FP qx_, FP qy_, FP qz_, FP gmx, FP gmy, FP gA, FP gB, FP gC, FP gp[3], FP gs[3],
                                                FP gq[4], FP& cov_trace, GeomCameraTerms<FP>* cam_terms = nullptr,
                                                FP aa_go = FP(0.0), FP* aa_rho = nullptr)
{
    // ---- geometry: recompute the forward quantities (gs_math.hpp order is irrelevant for the derivative)
    FP v[3];
    v[0] = FP((cp.right[0])) * px + FP((cp.right[1])) * py + FP((cp.right[2])) * pz + FP(cp.tx);
    v[1] = FP((cp.up[0])) * px + FP((cp.up[1])) * py + FP((cp.up[2])) * pz + FP(cp.ty);
    v[2] = FP((cp.front[0])) * px + FP((cp.front[1])) * py + FP((cp.front[2])) * pz + FP(cp.tz);
    const FP limx = FP(1.3) * FP(cp.tanfovx), limy = FP(1.3) * FP(cp.tanfovy);
    const FP rx = v[0] / v[2], ry = v[1] / v[2];
    const int   clx = (rx < -limx) ? -1 : (rx > limx ? 1 : 0);
    const int   cly = (ry < -limy) ? -1 : (ry > limy ? 1 : 0);
    const FP tx = (clx ? FP(clx) * limx : rx) * v[2];
    const FP ty = (cly ? FP(cly) * limy : ry) * v[2];
    const FP tz = v[2];
    const FP sc[3] = { scale_modifier * sc0, scale_modifier * sc1, scale_modifier * sc2 };
    const FP x = qx_, y = qy_, z = qz_, w = qw_;
    FP Rm[3][3];
    Rm[0][0] = FP(1.0) - FP(2.0) * y * y - FP(2.0) * z * z; Rm[0][1] = FP(2.0) * x * y - FP(2.0) * z * w; Rm[0][2] = FP(2.0) * x * z + FP(2.0) * y * w;
    Rm[1][0] = FP(2.0) * x * y + FP(2.0) * z * w; Rm[1][1] = FP(1.0) - FP(2.0) * x * x - FP(2.0) * z * z; Rm[1][2] = FP(2.0) * y * z - FP(2.0) * x * w;
    Rm[2][0] = FP(2.0) * x * z - FP(2.0) * y * w; Rm[2][1] = FP(2.0) * y * z + FP(2.0) * x * w; Rm[2][2] = FP(1.0) - FP(2.0) * x * x - FP(2.0) * y * y;
    FP M[3][3], Sig[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[r][k] = Rm[r][k] * sc[k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) Sig[r][k] = M[r][0] * M[k][0] + M[r][1] * M[k][1] + M[r][2] * M[k][2];
    const FP j00 = FP(cp.focalx) / tz, j11 = FP(cp.focaly) / tz, j02 = -FP(cp.focalx) * tx / (tz * tz),
                j12 = -FP(cp.focaly) * ty / (tz * tz);
    FP T0[3], T1[3], ST0[3], ST1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        T0[r] = FP(cp.right[r]) * j00 + FP(cp.front[r]) * j02;
        T1[r] = FP(cp.up[r]) * j11 + FP(cp.front[r]) * j12;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        ST0[r] = Sig[r][0] * T0[0] + Sig[r][1] * T0[1] + Sig[r][2] * T0[2];
        ST1[r] = Sig[r][0] * T1[0] + Sig[r][1] * T1[1] + Sig[r][2] * T1[2];
    }
    const FP a0 = T0[0] * ST0[0] + T0[1] * ST0[1] + T0[2] * ST0[2];
    const FP b = T1[0] * ST0[0] + T1[1] * ST0[1] + T1[2] * ST0[2];
    const FP c0 = T1[0] * ST1[0] + T1[1] * ST1[1] + T1[2] * ST1[2];
    const FP a = a0 + FP(0.3), c = c0 + FP(0.3);
    const FP D = a * c - b * b + FP(1e-6);
    const FP iD2 = FP(1.0) / (D * D);
    FP g00 = (-c * c * gA + b * c * gB + (D - a * c) * gC) * iD2;
    FP g11 = ((D - a * c) * gA + a * b * gB - a * a * gC) * iD2;
    FP g01 = (FP(2.0) * b * c * gA - (D + FP(2.0) * b * b) * gB + FP(2.0) * a * b * gC) * iD2;
    if (aa_rho) { // (a row of an antialiased frame; a compile-time NULL in the classic frame's kernels)
        const FP d0 = a0 * c0 - b * b, d1 = a * c - b * b;
        const FP q   = d0 / d1;
        const FP rho = q > FP(0.0) ? FP(sqrt(q)) : FP(0.0); // (a NaN quotient gives 0, like the forward)
        *aa_rho      = rho;
        if (rho > FP(0.0)) {
            const FP k = aa_go / (FP(2.0) * rho * (d1 * d1));
            g00 += k * (c0 * d1 - d0 * c);
            g11 += k * (a0 * d1 - d0 * a);
            g01 += k * (FP(2.0) * b * (d0 - d1));
        }
    }
    FP Gm[3][3], dT0[3], dT1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) Gm[r][k] = g00 * T0[r] * T0[k] + g01 * T1[r] * T0[k] + g11 * T1[r] * T1[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        dT0[r] = FP(2.0) * g00 * ST0[r] + g01 * ST1[r];
        dT1[r] = FP(2.0) * g11 * ST1[r] + g01 * ST0[r];
    }
    const FP dj00 = FP(cp.right[0]) * dT0[0] + FP(cp.right[1]) * dT0[1] + FP(cp.right[2]) * dT0[2];
    const FP dj02 = FP(cp.front[0]) * dT0[0] + FP(cp.front[1]) * dT0[1] + FP(cp.front[2]) * dT0[2];
    const FP dj11 = FP(cp.up[0]) * dT1[0] + FP(cp.up[1]) * dT1[1] + FP(cp.up[2]) * dT1[2];
    const FP dj12 = FP(cp.front[0]) * dT1[0] + FP(cp.front[1]) * dT1[1] + FP(cp.front[2]) * dT1[2];
    const FP itz2 = FP(1.0) / (tz * tz), itz3 = itz2 / tz;
    const FP dtx = dj02 * (-FP(cp.focalx) * itz2);
    const FP dty = dj12 * (-FP(cp.focaly) * itz2);
    const FP dtz = dj00 * (-FP(cp.focalx) * itz2) + dj11 * (-FP(cp.focaly) * itz2) + dj02 * (FP(2.0) * FP(cp.focalx) * tx * itz3) +
                      dj12 * (FP(2.0) * FP(cp.focaly) * ty * itz3);
    FP dv[3];
    dv[0] = clx ? FP(0.0) : dtx;
    dv[1] = cly ? FP(0.0) : dty;
    dv[2] = dtz + (clx ? dtx * FP(clx) * limx : FP(0.0)) + (cly ? dty * FP(cly) * limy : FP(0.0));
    const FP pw = FP(1.0) / (v[2] + FP(1e-6));
    dv[0] += gmx * FP(cp.focalx) * pw;
    dv[1] += gmy * FP(cp.focaly) * pw;
    dv[2] += -(gmx * FP(cp.focalx) * v[0] + gmy * FP(cp.focaly) * v[1]) * pw * pw;
#pragma unroll
    for (int i = 0; i < 3; ++i) gp[i] = FP(cp.right[i]) * dv[0] + FP(cp.up[i]) * dv[1] + FP(cp.front[i]) * dv[2];
    if (cam_terms) { // (camera_grad.hip; a compile-time NULL in the parameter pass)
#pragma unroll
        for (int i = 0; i < 3; ++i) cam_terms->dv[i] = dv[i], cam_terms->dT0[i] = dT0[i], cam_terms->dT1[i] = dT1[i];
        cam_terms->j00 = j00, cam_terms->j11 = j11, cam_terms->j02 = j02, cam_terms->j12 = j12;
    }

    FP dM[3][3], dRm[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            dM[r][k] = (Gm[r][0] + Gm[0][r]) * M[0][k] + (Gm[r][1] + Gm[1][r]) * M[1][k] + (Gm[r][2] + Gm[2][r]) * M[2][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gs[k] = scale_modifier * (dM[0][k] * Rm[0][k] + dM[1][k] * Rm[1][k] + dM[2][k] * Rm[2][k]);
#pragma unroll
        for (int r = 0; r < 3; ++r) dRm[r][k] = dM[r][k] * sc[k];
    }
    const FP gx_ = FP(2.0) * (y * (dRm[0][1] + dRm[1][0]) + z * (dRm[0][2] + dRm[2][0]) + w * (dRm[2][1] - dRm[1][2])) - FP(4.0) * x * (dRm[1][1] + dRm[2][2]);
    const FP gy_ = FP(2.0) * (x * (dRm[0][1] + dRm[1][0]) + z * (dRm[1][2] + dRm[2][1]) + w * (dRm[0][2] - dRm[2][0])) - FP(4.0) * y * (dRm[0][0] + dRm[2][2]);
    const FP gz_ = FP(2.0) * (x * (dRm[0][2] + dRm[2][0]) + y * (dRm[1][2] + dRm[2][1]) + w * (dRm[1][0] - dRm[0][1])) - FP(4.0) * z * (dRm[0][0] + dRm[1][1]);
    const FP gw_ = FP(2.0) * (z * (dRm[1][0] - dRm[0][1]) + y * (dRm[0][2] - dRm[2][0]) + x * (dRm[2][1] - dRm[1][2]));

    gq[0] = gw_; gq[1] = gx_; gq[2] = gy_; gq[3] = gz_; // (r, x, y, z)
    cov_trace = a + c;
}

// The global operands of survivor `vsafe` (dense id; lanes past V pass the last survivor's and discard the result), splat idx:
// its 2-D gradient row and its pos / scale / rotq rows.  Everything is requested here, together: one memory round trip per
// block instead of one per use.
struct SplatOperands {
    float  gmx, gmy, gA, gB, gC, gop, gcol[3]; // dL/d{pixel mean, conic, opacity, colour}
    float  px, py, pz, sc0, sc1, sc2;
    float4 q; // (r,x,y,z)
    float  opac; // the splat's own opacity: loaded for a row of an antialiased frame only (0 otherwise, never read)
};
// AA: a row of an antialiased frame (CamParams::raster_mode; the kernels are compiled once per mode, so the classic frame's
// pass is the code it was before the mode existed); opacity: the scene's rows, read only then
template <bool AA>
__device__ __forceinline__ SplatOperands load_splat_operands(uint32_t vsafe, int idx, const float* grads2d, const float* pos,
                                                             const float* scale, const float* rotq, const float* opacity)
{
    const float4* g2 = reinterpret_cast<const float4*>(grads2d + (size_t)vsafe * kG2D);
    const float4  q0 = g2[0], q1 = g2[1];
    const float   gcol2 = reinterpret_cast<const float*>(g2)[8];
    SplatOperands in;
    in.px = pos[3 * (size_t)idx + 0], in.py = pos[3 * (size_t)idx + 1], in.pz = pos[3 * (size_t)idx + 2];
    in.sc0 = scale[3 * (size_t)idx + 0], in.sc1 = scale[3 * (size_t)idx + 1], in.sc2 = scale[3 * (size_t)idx + 2];
    in.q = *reinterpret_cast<const float4*>(rotq + 4 * (size_t)idx);
    in.gmx = q0.x, in.gmy = q0.y, in.gA = q0.z, in.gB = q0.w, in.gC = q1.x, in.gop = q1.y;
    in.gcol[0] = q1.z, in.gcol[1] = q1.w, in.gcol[2] = gcol2;
    in.opac = AA ? opacity[idx] : 0.0f;
    return in;
}

// ---- what the per-row kernels (backward.hip's three preprocess passes, camera_grad.hip) share around those expressions
// One lane's place in block `blk` (256 rows) of a pass over the survivors [v0, V): its dense id (lanes past V take the last
// survivor's operands through vsafe and discard the result), its splat, and its wave's first dense id and number of live rows
struct RowBlock {
    uint32_t vid, vsafe, wave_first, nvalid;
    bool     valid;
    int      idx;
};
__device__ __forceinline__ RowBlock row_block(uint32_t v0, uint32_t V, uint32_t blk, const uint32_t* vis_index)
{
    RowBlock b;
    b.vid        = v0 + blk * 256u + threadIdx.x;
    b.valid      = b.vid < V;
    b.vsafe      = b.valid ? b.vid : V - 1;
    b.idx        = (int)vis_index[b.vsafe];
    b.wave_first = v0 + blk * 256u + (threadIdx.x >> 6) * 64u;
    b.nvalid     = b.wave_first < V ? ((V - b.wave_first) < 64u ? (V - b.wave_first) : 64u) : 0u;
    return b;
}
// "12 consecutive lanes own one splat's 192 bytes": step i (of 12) of a wave's pass over the 12 float4 of each of its 64 rows.
// body(slot, part, sidx) runs on the lanes of live rows: slot = the row inside the wave, part = its float4, sidx = its splat.
// (The loop over i and its unrolling are the caller's, and so is how the body captures: these kernels' register allocation
// follows such details, and each use is held to the registers its own copy of the loop had.)
template <class Body>
__device__ __forceinline__ void row_part_step(const RowBlock& b, int lane, int i, Body body)
{
    const uint32_t c    = (uint32_t)i * 64u + lane;
    const uint32_t slot = c / 12u, part = c - slot * 12u;
    const int      sidx = __shfl(b.idx, (int)slot, 64);
    if (slot < b.nvalid) body(slot, part, sidx);
}
// A footprint beyond this (trace of the 2-D covariance, px^2: radius ~ 3 sqrt(lambda_max) > 64 px) takes the algebra in f64.
constexpr float kGiantCovTrace = 455.0f;
// (Both precisions are inlined: the kernels' register count doubles and their occupancy halves -- preprocess-backward
//  0.181 -> 0.185 ms on the bicycle stand-in.  Holding them to the f32 occupancy with __launch_bounds__ spills the f64 branch
//  to scratch and costs 0.05 ms: measured in a same-box A/B.)

// The f32 algebra, and -- for screen-filling splats only -- the same algebra again in f64.  Their 2-D covariance is ~1e5 and
// their conic ~1e-6: conic -> covariance -> Sigma -> scale / quaternion multiplies sums that cancel to a 1e-3..1e-5 of their
// terms, and ANY f32 evaluation loses them (the f32 CPU restatement is off by up to 1.7e-1 on such rows; the 2-D gradients
// feeding this step are good to ~1e-4: profiles/r04_gradient_error_survey.txt).  0.4 % of the on-screen splats of the
// bicycle stand-in qualify; the kernels calling this are HBM-bound, the divergent f64 pass hides under their stores.
// gop: dL/dopacity of the row -- in.gop, times rho for a row of an antialiased frame (whose in.gop is dL/d(opacity rho)).
template <bool AA>
__device__ __forceinline__ void geom_backward(const CamParams& cp, float scale_modifier, const SplatOperands& in, float gp[3],
                                              float gs[3], float4& gq, float& gop)
{
    constexpr bool aa = AA;
    float dp[3], q4[4], tr, rho = 1.0f;
    geom_backward_t<float>(cp, scale_modifier, in.px, in.py, in.pz, in.sc0, in.sc1, in.sc2, in.q.x, in.q.y, in.q.z, in.q.w, in.gmx,
                           in.gmy, in.gA, in.gB, in.gC, dp, gs, q4, tr, nullptr, in.gop * in.opac, aa ? &rho : nullptr);
    if (tr > kGiantCovTrace) {
        double dpd[3], gsd[3], q4d[4], trd, rhod = 1.0;
        geom_backward_t<double>(cp, scale_modifier, in.px, in.py, in.pz, in.sc0, in.sc1, in.sc2, in.q.x, in.q.y, in.q.z, in.q.w,
                                in.gmx, in.gmy, in.gA, in.gB, in.gC, dpd, gsd, q4d, trd, nullptr, (double)in.gop * (double)in.opac,
                                aa ? &rhod : nullptr);
        rho = (float)rhod;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dp[i] = (float)dpd[i];
            gs[i] = (float)gsd[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) q4[i] = (float)q4d[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) gp[i] += dp[i];
    gq  = make_float4(q4[0], q4[1], q4[2], q4[3]);
    gop = aa ? in.gop * rho : in.gop;
}

// The colour step of that path for one splat: parks the 16 basis values of its view direction and its 3 clamp-masked
// dL/dcolour in its slab slot `mine`, and returns the direction part of dL/dpos (from the kept Jacobian rows j0..j2) in gp.
// (PARK = false: the direction part alone, nothing parked -- camera_grad.hip)
template <bool PARK = true>
__device__ __forceinline__ void jac_colour_step(const CamParams& cp, const SplatOperands& in, float4 j0, float4 j1, float4 j2,
                                                float* mine, float gp[3])
{
    const uint32_t mask = __float_as_uint(j2.y);
    const float*   gcol = in.gcol;
    const float dx = in.px - cp.campos[0], dy = in.py - cp.campos[1], dz = in.pz - cp.campos[2];
    const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
    const float x = dx * inv, y = dy * inv, z = dz * inv;
    const float xx = x * x, yy = y * y, zz = z * z;
    if (PARK) {
#define LCGS_BASIS(k, B, DX, DY, DZ) mine[k] = (B);
        LCGS_SH_TERMS(LCGS_BASIS)
#undef LCGS_BASIS
#pragma unroll
        for (int c = 0; c < 3; ++c) mine[16 + c] = ((mask >> c) & 1u) ? gcol[c] : 0.0f; // clamp mask
    }
    // J rows of clamped channels are already zero: no mask needed here
    const float ddx = gcol[0] * j0.x + gcol[1] * j0.w + gcol[2] * j1.z;
    const float ddy = gcol[0] * j0.y + gcol[1] * j1.x + gcol[2] * j1.w;
    const float ddz = gcol[0] * j0.z + gcol[1] * j1.y + gcol[2] * j2.x;
    const float dd  = x * ddx + y * ddy + z * ddz;
    gp[0] = (ddx - x * dd) * inv;
    gp[1] = (ddy - y * dd) * inv;
    gp[2] = (ddz - z * dd) * inv;
}

// The colour step from the coefficient rows themselves (frames without the kept Jacobian): `row` holds the splat's 48
// coefficients (zeros past 3 x feat); ADDS the direction part of dL/dpos to gp and, when STORE, replaces the row IN PLACE with
// the splat's SH gradient row (clamp-masked dL/dcolour x basis).
template <bool STORE>
__device__ __forceinline__ void sh_colour_step(const CamParams& cp, const SplatOperands& in, int feat, float* row, float gp[3])
{
    const float dx = in.px - cp.campos[0], dy = in.py - cp.campos[1], dz = in.pz - cp.campos[2];
    const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
    const float x = dx * inv, y = dy * inv, z = dz * inv;
    const float xx = x * x, yy = y * y, zz = z * z;
    float raw[3] = { 0.5f, 0.5f, 0.5f };
#define LCGS_RAW(k, B, DX, DY, DZ)                                                                                    \
    if (k < feat) {                                                                                                   \
        const float bk = (B);                                                                                         \
        raw[0] += bk * row[k * 3 + 0];                                                                                \
        raw[1] += bk * row[k * 3 + 1];                                                                                \
        raw[2] += bk * row[k * 3 + 2];                                                                                \
    }
    LCGS_SH_TERMS(LCGS_RAW)
#undef LCGS_RAW
    float g[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) g[ch] = (raw[ch] > 0.0f && raw[ch] < 1.0f) ? in.gcol[ch] : 0.0f; // clamp mask
    float ddx = 0.0f, ddy = 0.0f, ddz = 0.0f;
#define LCGS_GRAD(k, B, DX, DY, DZ)                                                                                   \
    {                                                                                                                 \
        const float c0 = row[k * 3 + 0], c1 = row[k * 3 + 1], c2 = row[k * 3 + 2];                                    \
        const float bk = (k < feat) ? (B) : 0.0f;                                                                     \
        const float wk = (k < feat) ? g[0] * c0 + g[1] * c1 + g[2] * c2 : 0.0f;                                       \
        ddx += wk * (DX);                                                                                             \
        ddy += wk * (DY);                                                                                             \
        ddz += wk * (DZ);                                                                                             \
        if (STORE) {                                                                                                  \
            row[k * 3 + 0] = bk * g[0];                                                                               \
            row[k * 3 + 1] = bk * g[1];                                                                               \
            row[k * 3 + 2] = bk * g[2];                                                                               \
        }                                                                                                             \
    }
    LCGS_SH_TERMS(LCGS_GRAD)
#undef LCGS_GRAD
    const float dd = x * ddx + y * ddy + z * ddz;
    gp[0] += (ddx - x * dd) * inv;
    gp[1] += (ddy - y * dd) * inv;
    gp[2] += (ddz - z * dd) * inv;
}

// One on-screen splat's twelve terms of the camera gradient (include/lcgs_hip.h "Camera gradient"), in the order of
// lcgs_camera's members: position, front, up, right.  gdir: the colour step's direction part of dL/dpos; gz: the depth
// channel's dL/dz (0 without one).  With d = pos - position:
//   position -= right dv0 + up dv1 + front dv2 + gdir        right += dv0 d + j00 dT0
//   up       += dv1 d + j11 dT1                              front += dv2 d + j02 dT0 + j12 dT1
template <typename FP>
__device__ __forceinline__ void camera_terms_t(const CamParams& cp, const SplatOperands& in, const GeomCameraTerms<FP>& t,
                                               const float gdir[3], float gz, double out[12])
{
    const FP d[3] = { FP(in.px) - FP(cp.campos[0]), FP(in.py) - FP(cp.campos[1]), FP(in.pz) - FP(cp.campos[2]) };
    const FP dv2  = t.dv[2] + FP(gz);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[0 + i] = (double)(-(FP(cp.right[i]) * t.dv[0] + FP(cp.up[i]) * t.dv[1] + FP(cp.front[i]) * dv2 + FP(gdir[i])));
        out[3 + i] = (double)(dv2 * d[i] + t.j02 * t.dT0[i] + t.j12 * t.dT1[i]);
        out[6 + i] = (double)(t.dv[1] * d[i] + t.j11 * t.dT1[i]);
        out[9 + i] = (double)(t.dv[0] * d[i] + t.j00 * t.dT0[i]);
    }
}
// ... in the precision geom_backward takes for this splat: binary32, binary64 for a screen-filling footprint
template <bool AA>
__device__ __forceinline__ void camera_terms(const CamParams& cp, float scale_modifier, const SplatOperands& in,
                                             const float gdir[3], float gz, double out[12])
{
    constexpr bool         aa = AA; // (an antialiased frame: the compensation's covariance term, as geom_backward)
    float                  dp[3], gs[3], q4[4], tr, rho;
    GeomCameraTerms<float> t;
    geom_backward_t<float>(cp, scale_modifier, in.px, in.py, in.pz, in.sc0, in.sc1, in.sc2, in.q.x, in.q.y, in.q.z, in.q.w, in.gmx,
                           in.gmy, in.gA, in.gB, in.gC, dp, gs, q4, tr, &t, in.gop * in.opac, aa ? &rho : nullptr);
    if (tr > kGiantCovTrace) {
        double                  dpd[3], gsd[3], q4d[4], trd, rhod;
        GeomCameraTerms<double> td;
        geom_backward_t<double>(cp, scale_modifier, in.px, in.py, in.pz, in.sc0, in.sc1, in.sc2, in.q.x, in.q.y, in.q.z, in.q.w,
                                in.gmx, in.gmy, in.gA, in.gB, in.gC, dpd, gsd, q4d, trd, &td, (double)in.gop * (double)in.opac,
                                aa ? &rhod : nullptr);
        camera_terms_t<double>(cp, in, td, gdir, gz, out);
    } else {
        camera_terms_t<float>(cp, in, t, gdir, gz, out);
    }
}

} // namespace lcgs

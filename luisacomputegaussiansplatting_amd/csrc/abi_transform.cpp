// abi_transform.cpp -- the C ABI, part 10: a similarity transform of a scene (csrc/kernels/transform.hip) -- the plan (host,
// binary64: the rotation's quaternion and its matrix on each SH band in the basis of gs_math.hpp's LCGS_SH_TERMS), the camera
// that goes with a transformed scene, the transform of the activated arrays, and the keep mask of a crop box.
#include <math.h>
#include <string.h>

#include "abi_internal.hpp"

using namespace lcgs;
using namespace lcgs::abi;

static_assert(sizeof(lcgs_similarity_plan) == sizeof(TransformPlan), "the kernels' plan is the header's, member for member");

namespace
{
// ---- the SH basis of one band as polynomials: LCGS_SH_TERMS' expressions, monomial by monomial.  The constants are the
// literals of gs_math.hpp read as binary64 (the orthonormal real harmonics to 1e-16): D_l is then orthogonal to rounding.
constexpr double kC1 = 0.4886025119029199;
constexpr double kC2[5] = { 1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396 };
constexpr double kC3[7] = { -0.5900435899266435, 2.890611442640554,  -0.4570457994644658, 0.3731763325901154,
                            -0.4570457994644658, 1.445305721320277,  -0.5900435899266435 };
struct Mono {
    int    a, b, c; // x^a y^b z^c
    double k;
};
struct Term {
    double C;
    int    n;
    Mono   m[3];
};
const Term kBand1[3] = { { -kC1, 1, { { 0, 1, 0, 1 } } }, { kC1, 1, { { 0, 0, 1, 1 } } }, { -kC1, 1, { { 1, 0, 0, 1 } } } };
const Term kBand2[5] = { { kC2[0], 1, { { 1, 1, 0, 1 } } },
                         { kC2[1], 1, { { 0, 1, 1, 1 } } },
                         { kC2[2], 3, { { 0, 0, 2, 2 }, { 2, 0, 0, -1 }, { 0, 2, 0, -1 } } },
                         { kC2[3], 1, { { 1, 0, 1, 1 } } },
                         { kC2[4], 2, { { 2, 0, 0, 1 }, { 0, 2, 0, -1 } } } };
const Term kBand3[7] = { { kC3[0], 2, { { 2, 1, 0, 3 }, { 0, 3, 0, -1 } } },
                         { kC3[1], 1, { { 1, 1, 1, 1 } } },
                         { kC3[2], 3, { { 0, 1, 2, 4 }, { 2, 1, 0, -1 }, { 0, 3, 0, -1 } } },
                         { kC3[3], 3, { { 0, 0, 3, 2 }, { 2, 0, 1, -3 }, { 0, 2, 1, -3 } } },
                         { kC3[4], 3, { { 1, 0, 2, 4 }, { 3, 0, 0, -1 }, { 1, 2, 0, -1 } } },
                         { kC3[5], 2, { { 2, 0, 1, 1 }, { 0, 2, 1, -1 } } },
                         { kC3[6], 2, { { 3, 0, 0, 1 }, { 1, 2, 0, -3 } } } };

// D_l for the rotation Rh (row-major), row-major D[k][j] with B_k(Rh d) = sum_j D[k][j] B_j(d).  A band's functions are
// homogeneous harmonic polynomials of degree l, i.e. symmetric tensors T_k of rank l (B_k(d) = T_k d ... d); rotating the
// argument rotates every index, and under the full contraction <.,.> (a rotation-invariant inner product, so the band's
// functions are orthogonal under it as they are on the sphere)  D[k][j] = (C_k / C_j) <T_k o Rh, T_j> / <T_j, T_j>, the
// tensors taken WITHOUT the constants and scaled by l!: small integers, so for a signed permutation matrix every sum is exact
// and the identity gives the identity.  No linear solve, nothing sampled.
template <int L>
void band_matrix(const Term* band, const double Rh[9], double* D)
{
    constexpr int N = 2 * L + 1, E = L == 1 ? 3 : L == 2 ? 9 : 27;
    const double  fact[4] = { 1, 1, 2, 6 };
    double        T[N][E], TR[N][E];
    for (int k = 0; k < N; ++k)
        for (int e = 0; e < E; ++e) {
            int cnt[3] = { 0, 0, 0 };
            for (int n = 0, r = e; n < L; ++n, r /= 3) ++cnt[r % 3];
            double v = 0.0;
            for (int m = 0; m < band[k].n; ++m) {
                const Mono& mo = band[k].m[m];
                if (mo.a == cnt[0] && mo.b == cnt[1] && mo.c == cnt[2]) v = mo.k * (fact[mo.a] * fact[mo.b] * fact[mo.c]);
            }
            T[k][e] = v;
        }
    for (int k = 0; k < N; ++k) {
        double cur[E], nxt[E];
        for (int e = 0; e < E; ++e) cur[e] = T[k][e];
        for (int mode = 0, stride = 1; mode < L; ++mode, stride *= 3) { // index `mode` of the tensor: i -> a through Rh[i][a]
            for (int e = 0; e < E; ++e) {
                const int a = (e / stride) % 3, base = e - a * stride;
                double    s = 0.0;
                for (int i = 0; i < 3; ++i) s += cur[base + i * stride] * Rh[3 * i + a];
                nxt[e] = s;
            }
            for (int e = 0; e < E; ++e) cur[e] = nxt[e];
        }
        for (int e = 0; e < E; ++e) TR[k][e] = cur[e];
    }
    for (int k = 0; k < N; ++k)
        for (int j = 0; j < N; ++j) {
            double num = 0.0, den = 0.0;
            for (int e = 0; e < E; ++e) num += TR[k][e] * T[j][e], den += T[j][e] * T[j][e];
            D[k * N + j] = (band[k].C * (num / den)) / band[j].C + 0.0; // (+ 0.0: a zero entry is +0)
        }
}

struct Plan64 {
    double Rh[9], q[4] /* w x y z */, s, t[3], D[83];
};

lcgs_status make_plan64(const lcgs_similarity* xf, Plan64* p)
{
    LCGS_REQUIRE(xf != nullptr, "NULL similarity");
    bool finite = isfinite(xf->scale);
    for (int i = 0; i < 9; ++i) finite = finite && isfinite(xf->rot[i]);
    for (int i = 0; i < 3; ++i) finite = finite && isfinite(xf->trans[i]);
    LCGS_REQUIRE(finite, "similarity: a non-finite value in rot, scale or trans");
    LCGS_REQUIRE(xf->scale > 0.0f, "similarity: scale must be > 0 (non-uniform scale and reflections are not offered)");
    double r[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[i][j] = (double)xf->rot[3 * i + j];
    double defect = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = ((r[i][0] * r[j][0] + r[i][1] * r[j][1]) + r[i][2] * r[j][2]) - (i == j ? 1.0 : 0.0);
            defect         = fmax(defect, fabs(g));
        }
    LCGS_REQUIRE(defect <= 1e-4, "similarity: rot is not a rotation, max |rot rot^T - I| > 1e-4");
    const double det = (r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) - r[0][1] * (r[1][0] * r[2][2] - r[1][2] * r[2][0])) +
                       r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]);
    LCGS_REQUIRE(det > 0.0, "similarity: det rot <= 0 (a reflection has no quaternion)");
    // Shepperd's method: the largest of the trace and the diagonal picks the component that is taken by a square root
    const double tr = (r[0][0] + r[1][1]) + r[2][2];
    double       w, x, y, z;
    if (tr >= r[0][0] && tr >= r[1][1] && tr >= r[2][2]) {
        w = 0.5 * sqrt(1.0 + tr);
        const double k = 0.25 / w;
        x = (r[2][1] - r[1][2]) * k, y = (r[0][2] - r[2][0]) * k, z = (r[1][0] - r[0][1]) * k;
    } else if (r[0][0] >= r[1][1] && r[0][0] >= r[2][2]) {
        x = 0.5 * sqrt(((1.0 + r[0][0]) - r[1][1]) - r[2][2]);
        const double k = 0.25 / x;
        w = (r[2][1] - r[1][2]) * k, y = (r[0][1] + r[1][0]) * k, z = (r[0][2] + r[2][0]) * k;
    } else if (r[1][1] >= r[2][2]) {
        y = 0.5 * sqrt(((1.0 - r[0][0]) + r[1][1]) - r[2][2]);
        const double k = 0.25 / y;
        w = (r[0][2] - r[2][0]) * k, x = (r[0][1] + r[1][0]) * k, z = (r[1][2] + r[2][1]) * k;
    } else {
        z = 0.5 * sqrt(((1.0 - r[0][0]) - r[1][1]) + r[2][2]);
        const double k = 0.25 / z;
        w = (r[1][0] - r[0][1]) * k, x = (r[0][2] + r[2][0]) * k, y = (r[1][2] + r[2][1]) * k;
    }
    const double n = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / n, x = x / n, y = y / n, z = z / n;
    if (w < 0.0) w = -w, x = -x, y = -y, z = -z; // q and -q are one rotation: the one with w >= 0
    p->q[0] = w, p->q[1] = x, p->q[2] = y, p->q[3] = z;
    // gs_math.hpp rot_from_quat's expressions (there column-major), the rotation every array sees
    double* R = p->Rh;
    R[0] = 1.0 - 2.0 * y * y - 2.0 * z * z;
    R[3] = 2.0 * x * y + 2.0 * z * w;
    R[6] = 2.0 * x * z - 2.0 * y * w;
    R[1] = 2.0 * x * y - 2.0 * z * w;
    R[4] = 1.0 - 2.0 * x * x - 2.0 * z * z;
    R[7] = 2.0 * y * z + 2.0 * x * w;
    R[2] = 2.0 * x * z + 2.0 * y * w;
    R[5] = 2.0 * y * z - 2.0 * x * w;
    R[8] = 1.0 - 2.0 * x * x - 2.0 * y * y;
    p->s = (double)xf->scale;
    for (int i = 0; i < 3; ++i) p->t[i] = (double)xf->trans[i];
    band_matrix<1>(kBand1, R, p->D);
    band_matrix<2>(kBand2, R, p->D + 9);
    band_matrix<3>(kBand3, R, p->D + 34);
    return LCGS_OK;
}

bool overlaps(const float* a, size_t a_floats, const float* b, size_t b_floats) { return a < b + b_floats && b < a + a_floats; }
} // namespace

extern "C" {

lcgs_status lcgs_similarity_plan_make(const lcgs_similarity* xf, lcgs_similarity_plan* out, double* D64)
{
    LCGS_REQUIRE(xf && out, "NULL argument");
    Plan64 p;
    LCGS_TRY(make_plan64(xf, &p));
    for (int i = 0; i < 9; ++i) out->M[i] = (float)(p.s * p.Rh[i]);
    for (int i = 0; i < 3; ++i) out->t[i] = xf->trans[i];
    out->s = xf->scale;
    for (int i = 0; i < 4; ++i) out->q[i] = (float)p.q[i];
    for (int i = 0; i < 9; ++i) out->D1[i] = (float)p.D[i];
    for (int i = 0; i < 25; ++i) out->D2[i] = (float)p.D[9 + i];
    for (int i = 0; i < 49; ++i) out->D3[i] = (float)p.D[34 + i];
    if (D64) memcpy(D64, p.D, sizeof(p.D));
    return LCGS_OK;
}

lcgs_status lcgs_camera_transform(const lcgs_camera* in, const lcgs_similarity* xf, lcgs_camera* out)
{
    LCGS_REQUIRE(in && xf && out, "NULL argument");
    Plan64 p;
    LCGS_TRY(make_plan64(xf, &p));
    const lcgs_camera c = *in; // (out may be in)
    auto rotate = [&](const float v[3], int i) {
        return (p.Rh[3 * i + 0] * (double)v[0] + p.Rh[3 * i + 1] * (double)v[1]) + p.Rh[3 * i + 2] * (double)v[2];
    };
    *out = c;
    for (int i = 0; i < 3; ++i) {
        out->position[i] = (float)(p.s * rotate(c.position, i) + p.t[i]);
        out->front[i]    = (float)rotate(c.front, i);
        out->up[i]       = (float)rotate(c.up, i);
        out->right[i]    = (float)rotate(c.right, i);
    }
    return LCGS_OK;
}

lcgs_status lcgs_scene_transform(lcgs_context* ctx, int num_gaussians, int sh_degree, const lcgs_similarity* xf,
                                 const lcgs_params* in, const lcgs_params* out)
{
    LCGS_REQUIRE(ctx && xf && in && out, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    LCGS_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "sh_degree must be in [0,3]");
    const float* const src[5] = { in->pos, in->scale, in->rotq, in->sh, in->opacity };
    float* const       dst[5] = { out->pos, out->scale, out->rotq, out->sh, out->opacity };
    for (int a = 0; a < 5; ++a) LCGS_REQUIRE(!dst[a] || src[a], "an output array is given but its input is NULL");
    lcgs_similarity_plan plan;
    LCGS_TRY(lcgs_similarity_plan_make(xf, &plan, nullptr));
    const RowFloats rowf = row_floats(sh_degree);
    size_t          floats[5];
    for (int a = 0; a < 5; ++a) floats[a] = rowf[a] * (size_t)std::max(num_gaussians, 1); // (aliasing is refused at any count)
    {
        bool aliased = false;
        for (int a = 0; a < 5; ++a) {
            if (!dst[a]) continue;
            for (int b = 0; b < 5; ++b) {
                if (!dst[b]) continue; // (neither read nor written)
                const bool in_place = a == b && dst[a] == src[b];
                aliased = aliased || (!in_place && overlaps(dst[a], floats[a], src[b], floats[b]));
                aliased = aliased || (b > a && overlaps(dst[a], floats[a], dst[b], floats[b]));
            }
        }
        LCGS_REQUIRE(!aliased, "an output may be its own input (in place); any other overlap of an output with an input or "
                               "another output is refused (alias)");
    }
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    // rows a context derived from arrays that are written here are dropped (every live context is looked at); a scene this
    // context has bound loses its f16 coefficient copy and the kept state of its last frame as well (lcgs_scene_modified)
    bool touched = false;
    {
        const float* const bound[5] = { ctx->pos, ctx->scale, ctx->rotq, ctx->sh, ctx->opacity };
        const RowFloats    bw       = row_floats(ctx->sh_deg);
        for (int a = 0; a < 5; ++a)
            for (int b = 0; b < 5; ++b)
                touched = touched || (dst[a] && bound[b] && ctx->P > 0 && overlaps(dst[a], floats[a], bound[b], bw[b] * (size_t)ctx->P));
    }
    scene_arrays_written(ctx, out->pos, out->scale, out->rotq);
    if (touched) {
        LCGS_TRY(join_aux_stream(ctx)); // (a pipelined frame's tail may still read the arrays)
        scene_modified_elsewhere(ctx);
        for (lcgs_context* c = ctx; c; c = c->twin) c->use_half_sh = false, c->last.valid = false;
    }
    TransformPlan tp;
    memcpy(&tp, &plan, sizeof(tp));
    launch_scene_transform(num_gaussians, sh_degree, tp, in->pos, in->scale, in->rotq, in->sh, out->pos, out->scale, out->rotq,
                           out->sh, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    const size_t P = (size_t)num_gaussians;
    if (out->sh && sh_degree == 0 && out->sh != in->sh)
        LCGS_HIP_CHECK(hipMemcpyAsync(out->sh, in->sh, P * 12, hipMemcpyDeviceToDevice, ctx->stream));
    if (out->opacity && out->opacity != in->opacity)
        LCGS_HIP_CHECK(hipMemcpyAsync(out->opacity, in->opacity, P * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (touched) return refresh_cull_bound(ctx); // (context-owned arrays: the rows are rebuilt behind the transform)
    return LCGS_OK;
}

lcgs_status lcgs_scene_box_keep_mask(lcgs_context* ctx, int num_gaussians, const float* d_pos, const lcgs_similarity* world_to_box,
                                     const float half_extent[3], uint8_t* d_keep)
{
    LCGS_REQUIRE(ctx && d_pos && world_to_box && half_extent && d_keep, "NULL argument");
    LCGS_REQUIRE(num_gaussians >= 0, "num_gaussians is negative");
    for (int k = 0; k < 3; ++k) LCGS_REQUIRE(half_extent[k] >= 0.0f, "half_extent must be >= 0 and not NaN (+inf: unbounded)");
    lcgs_similarity_plan plan;
    LCGS_TRY(lcgs_similarity_plan_make(world_to_box, &plan, nullptr));
    LCGS_ENTRY(ctx);
    if (num_gaussians == 0) return LCGS_OK;
    LCGS_HIP_CHECK(hipSetDevice(ctx->device));
    TransformPlan tp;
    memcpy(&tp, &plan, sizeof(tp));
    launch_box_keep_mask(num_gaussians, tp, d_pos, half_extent, d_keep, ctx->stream);
    LCGS_HIP_CHECK(hipGetLastError());
    return LCGS_OK;
}

} // extern "C"

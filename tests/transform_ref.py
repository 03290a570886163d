"""NumPy restatement of the scene similarity transform (include/lcgs_hip.h: lcgs_similarity_plan_make, lcgs_camera_transform,
lcgs_scene_transform, lcgs_scene_box_keep_mask) -- the yardstick of tests/test_transform_ref.py, tests/test_transform_abi.py and
tests/test_gpu_transform.py.  Nothing here calls the library.

  plan64      the plan in binary64: Shepperd's quaternion (w, x, y, z), normalised, w >= 0; Rhat rebuilt from it with
              rot_from_quat's expressions; the band matrices D_1, D_2, D_3 by a method of this file's own -- every basis function
              of LCGS_SH_TERMS as a polynomial {monomial: coefficient}, the rows of Rhat substituted for x, y, z by polynomial
              multiplication, and the result projected on the band with the apolar inner product <x^a y^b z^c, same> = a! b! c!
              (rotation invariant, so the band's functions are orthogonal under it), the constants applied last as C_k / C_j:
              no solve, nothing sampled, integer sums for a signed permutation
  plan32      each of M = s Rhat, t, s, q and the D_l rounded to binary32 once
  camera      position' = s Rhat position + t, front / up / right rotated, binary64
  transform   the row expressions of the header, in the header's operation order, in the dtype of the plan given
  box_keep    the crop's keep bytes
"""
import math

import numpy as np

U = 2.0 ** -24
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
# gs_math.hpp's literals, read as binary64
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
# LCGS_SH_TERMS 1..15 as (constant, {exponents of x y z: coefficient})
BANDS = {
    1: [(-C1, {Y: 1}), (C1, {Z: 1}), (-C1, {X: 1})],
    2: [(C2[0], {(1, 1, 0): 1}), (C2[1], {(0, 1, 1): 1}), (C2[2], {(0, 0, 2): 2, (2, 0, 0): -1, (0, 2, 0): -1}),
        (C2[3], {(1, 0, 1): 1}), (C2[4], {(2, 0, 0): 1, (0, 2, 0): -1})],
    3: [(C3[0], {(2, 1, 0): 3, (0, 3, 0): -1}), (C3[1], {(1, 1, 1): 1}), (C3[2], {(0, 1, 2): 4, (2, 1, 0): -1, (0, 3, 0): -1}),
        (C3[3], {(0, 0, 3): 2, (2, 0, 1): -3, (0, 2, 1): -3}), (C3[4], {(1, 0, 2): 4, (3, 0, 0): -1, (1, 2, 0): -1}),
        (C3[5], {(2, 0, 1): 1, (0, 2, 1): -1}), (C3[6], {(3, 0, 0): 1, (1, 2, 0): -3})],
}


def _mul(p, q):
    out = {}
    for (a, b, c), u in p.items():
        for (d, e, f), v in q.items():
            k = (a + d, b + e, c + f)
            out[k] = out.get(k, 0.0) + u * v
    return out


def _apolar(p, q):
    return sum(v * q[m] * math.factorial(m[0]) * math.factorial(m[1]) * math.factorial(m[2]) for m, v in p.items() if m in q)


def band_matrix(l, Rh):
    """D_l [2l+1, 2l+1] with B_l(Rh d) = D_l B_l(d)"""
    rows = [{X: float(Rh[i, 0]), Y: float(Rh[i, 1]), Z: float(Rh[i, 2])} for i in range(3)]  # (Rh d)_i as a polynomial in d
    basis = [{m: float(k) for m, k in mono.items()} for _, mono in BANDS[l]]  # (the constants are applied at the end)
    n = 2 * l + 1
    D = np.zeros((n, n))
    for k, (C, mono) in enumerate(BANDS[l]):
        rotated = {}
        for (a, b, c), coef in mono.items():
            term = {(0, 0, 0): float(coef)}
            for i, e in enumerate((a, b, c)):
                for _ in range(e):
                    term = _mul(term, rows[i])
            for m, v in term.items():
                rotated[m] = rotated.get(m, 0.0) + v
        for j in range(n):
            D[k, j] = (C * (_apolar(rotated, basis[j]) / _apolar(basis[j], basis[j]))) / BANDS[l][j][0] + 0.0
    return D


def quat_from_rot(r):
    """Shepperd's method on a [3, 3] binary64 matrix -> (w, x, y, z), normalised, w >= 0; the header's operation order"""
    r = [[float(r[i][j]) for j in range(3)] for i in range(3)]
    tr = (r[0][0] + r[1][1]) + r[2][2]
    if tr >= r[0][0] and tr >= r[1][1] and tr >= r[2][2]:
        w = 0.5 * math.sqrt(1.0 + tr)
        k = 0.25 / w
        x, y, z = (r[2][1] - r[1][2]) * k, (r[0][2] - r[2][0]) * k, (r[1][0] - r[0][1]) * k
    elif r[0][0] >= r[1][1] and r[0][0] >= r[2][2]:
        x = 0.5 * math.sqrt(((1.0 + r[0][0]) - r[1][1]) - r[2][2])
        k = 0.25 / x
        w, y, z = (r[2][1] - r[1][2]) * k, (r[0][1] + r[1][0]) * k, (r[0][2] + r[2][0]) * k
    elif r[1][1] >= r[2][2]:
        y = 0.5 * math.sqrt(((1.0 - r[0][0]) + r[1][1]) - r[2][2])
        k = 0.25 / y
        w, x, z = (r[0][2] - r[2][0]) * k, (r[0][1] + r[1][0]) * k, (r[1][2] + r[2][1]) * k
    else:
        z = 0.5 * math.sqrt(((1.0 - r[0][0]) - r[1][1]) + r[2][2])
        k = 0.25 / z
        w, x, y = (r[1][0] - r[0][1]) * k, (r[0][2] + r[2][0]) * k, (r[1][2] + r[2][1]) * k
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    return w, x, y, z


def rot_from_quat(w, x, y, z):
    """gs_math.hpp rot_from_quat's expressions, as a row-major matrix"""
    return np.array([[1.0 - 2.0 * y * y - 2.0 * z * z, 2.0 * x * y - 2.0 * z * w, 2.0 * x * z + 2.0 * y * w],
                     [2.0 * x * y + 2.0 * z * w, 1.0 - 2.0 * x * x - 2.0 * z * z, 2.0 * y * z - 2.0 * x * w],
                     [2.0 * x * z - 2.0 * y * w, 2.0 * y * z + 2.0 * x * w, 1.0 - 2.0 * x * x - 2.0 * y * y]])


def plan64(rot, scale=1.0, trans=(0.0, 0.0, 0.0)):
    """the binary64 plan of the binary32 inputs (rot [3, 3] row-major)"""
    r = np.asarray(rot, np.float32).reshape(3, 3).astype(np.float64)
    s = float(np.float32(scale))
    t = np.asarray(trans, np.float32).astype(np.float64)
    q = quat_from_rot(r)
    Rh = rot_from_quat(*q)
    return {"q": np.array(q), "Rh": Rh, "s": s, "t": t, "M": s * Rh, "D": tuple(band_matrix(l, Rh) for l in (1, 2, 3))}


def plan32(p):
    f = np.float32
    return {"q": p["q"].astype(f), "s": f(p["s"]), "t": p["t"].astype(f), "M": p["M"].astype(f),
            "D": tuple(d.astype(f) for d in p["D"])}


def camera(cam, p):
    """cam: dict with position / front / up / right (+ the copied members) -> the same dict for the transformed scene, binary64"""
    rot = lambda v, i: (p["Rh"][i, 0] * v[0] + p["Rh"][i, 1] * v[1]) + p["Rh"][i, 2] * v[2]
    out = dict(cam)
    pos = [float(v) for v in cam["position"]]
    out["position"] = [p["s"] * rot(pos, i) + p["t"][i] for i in range(3)]
    for k in ("front", "up", "right"):
        v = [float(x) for x in cam[k]]
        out[k] = [rot(v, i) for i in range(3)]
    return out


def transform(scene, plan, sh_deg=3, rotate_sh=True):
    """the header's row expressions in the plan's dtype (plan32 -> the kernels' bits, plan64 -> the binary64 yardstick); scene: the
    activated arrays, any subset of KEYS; rotate_sh False: the coefficients are copied (what a tool that skips them does)"""
    dt = plan["M"].dtype.type
    M, t, s = plan["M"], plan["t"], dt(plan["s"])
    W, X_, Y_, Z_ = (dt(v) for v in plan["q"])
    out = {}
    with np.errstate(all="ignore"):
        if "pos" in scene:
            p = np.asarray(scene["pos"]).reshape(-1, 3).astype(dt)
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            out["pos"] = np.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + t[i] for i in range(3)], axis=1)
        if "scale" in scene:
            out["scale"] = s * np.asarray(scene["scale"]).reshape(-1, 3).astype(dt)
        if "rotq" in scene:
            q = np.asarray(scene["rotq"]).reshape(-1, 4).astype(dt)
            w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            out["rotq"] = np.stack([((W * w - X_ * x) - Y_ * y) - Z_ * z, ((W * x + X_ * w) + Y_ * z) - Z_ * y,
                                    ((W * y - X_ * z) + Y_ * w) + Z_ * x, ((W * z + X_ * y) - Y_ * x) + Z_ * w], axis=1)
        if "sh" in scene:
            K = (sh_deg + 1) ** 2
            c = np.asarray(scene["sh"]).astype(dt)
            shape = c.shape
            c = c.reshape(-1, K, 3)
            o = c.copy()
            for l in range(1, sh_deg + 1 if rotate_sh else 0):
                D, lo = plan["D"][l - 1], l * l
                for k in range(2 * l + 1):
                    acc = D[k, 0] * c[:, lo, :]
                    for j in range(1, 2 * l + 1):
                        acc = acc + D[k, j] * c[:, lo + j, :]
                    o[:, lo + k, :] = acc
            out["sh"] = o.reshape(shape)
        if "opacity" in scene:
            out["opacity"] = np.asarray(scene["opacity"]).astype(dt).copy()
    return out


def box_keep(pos, plan, half):
    """the keep bytes of lcgs_scene_box_keep_mask (plan: plan32 of world_to_box)"""
    with np.errstate(all="ignore"):
        b = transform({"pos": pos}, plan)["pos"]
        return (np.abs(b) <= np.asarray(half, np.float32)[None, :]).all(axis=1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- inputs
def random_rotation(rng):
    """a rotation matrix drawn from a random unit quaternion, rounded to binary32 (what a caller passes)"""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return rot_from_quat(*q).astype(np.float32)


def axis_turn(axis, degrees=90.0):
    a, c, s = np.radians(degrees), math.cos(np.radians(degrees)), math.sin(np.radians(degrees))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r.astype(np.float32)


def rotation_set():
    """20 seeded random rotations, the identity and the three 90-degree axis turns"""
    rng = np.random.default_rng(2024)
    return [random_rotation(rng) for _ in range(20)] + [np.eye(3, dtype=np.float32)] + [axis_turn(a) for a in range(3)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    view = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(view) == b.view(view)).all())

"""A second, independent reading of the reference's shading and path loop, in numpy f32.

Written from the reference source alone (file:line on every function), one f32 operation per
reference operation, in the reference's order; it shares no code with oracle/ or the HIP
library.  Conventions where the reference leaves a choice: arguments are
evaluated left to right; sin / cos / atan are the f64 library value rounded to f32; std::min and
std::max keep their ternary NaN behaviour; a null material and a Mix that resolves to Emissive end
the path; the clamp applies only when ray_clamp > 0.

Intersection is brute force over every triangle in global order, so nothing here depends on a BVH.
A ray whose closest hit is tied in exact f32 t between two triangles (other than exact duplicates of
one another), or that has an exactly-zero direction component, is builder dependent in the
reference; `Tracer.ambiguous` records it.

Vectors are tuples of np.float32 scalars.  Every arithmetic result is wrapped in F() so that the
precision does not depend on numpy's scalar promotion rules.
"""
import math
from collections import Counter

import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
np.seterr(all="ignore")

PI = F(3.1415926535897932384)          # common/math.h:37
PI2 = F(PI / F(2.0))                   # math.h:38
PI4 = F(PI / F(4.0))                   # math.h:39
INV_PI = F(F(1.0) / PI)                # math.h:40
EPS = F(0.001)                         # math.h:41
SHADOW_EPS = F(0.0001)                 # math.h:42
INF = F(np.inf)


# ----------------------------------------------------------------------------- scalar helpers
def fsin(x):
    return F(math.sin(float(x))) if math.isfinite(float(x)) else F(np.nan)


def fcos(x):
    return F(math.cos(float(x))) if math.isfinite(float(x)) else F(np.nan)


def fatan(x):
    return F(math.atan(float(x)))


def fsqrt(x):
    return F(np.sqrt(F(x)))


def fabs(x):
    return F(np.abs(F(x)))


def std_max(a, b):
    """std::max(a, b): (a < b) ? b : a."""
    return b if a < b else a


def std_min(a, b):
    """std::min(a, b): (b < a) ? b : a."""
    return b if b < a else a


def neg(v):
    return tuple(F(-x) for x in v)


def add(a, b):
    return tuple(F(x + y) for x, y in zip(a, b))


def sub(a, b):
    return tuple(F(x - y) for x, y in zip(a, b))


def mul(a, b):
    return tuple(F(x * y) for x, y in zip(a, b))


def scale(s, v):
    """scalar * Array and Array * scalar (common/array.h:156-162, 199): element-wise."""
    return tuple(F(F(s) * x) for x in v)


def divs(v, s):
    """Array / scalar (array.h:156-162): a true division per element."""
    return tuple(F(x / F(s)) for x in v)


def dot(a, b):
    """common/array.h:210-216: a0*b0, then += ai*bi in order."""
    s = F(a[0] * b[0])
    for i in range(1, len(a)):
        s = F(s + F(a[i] * b[i]))
    return s


def cross(a, b):
    """common/math.h:177-181."""
    return (F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])),
            F(F(a[0] * b[1]) - F(a[1] * b[0])))


def length(a):
    """array.h:280-282."""
    return fsqrt(dot(a, a))


def normalize(a):
    """array.h:284-286: a / sqrt(dot(a, a))."""
    return divs(a, fsqrt(dot(a, a)))


def lerp3(v0, v1, v2, uv):
    """math.h:49-51: (1 - uv0 - uv1) * v0 + uv0 * v1 + uv1 * v2."""
    w = F(F(F(1.0) - uv[0]) - uv[1])
    return add(add(scale(w, v0), scale(uv[0], v1)), scale(uv[1], v2))


def vec(a):
    return tuple(F(x) for x in a)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- sampler
class LCG:
    """LCGSampler, kernel/sampler.h:54-67."""

    def __init__(self, seed=0):
        self.seed = seed & M32

    def copy(self):
        return LCG(self.seed)

    def next1d(self):
        self.seed = (1103515245 * self.seed + 12345) & M32
        return F(F(self.seed) / F(0xFFFFFFFF))

    def next2d(self):
        a = self.next1d()
        return (a, self.next1d())


def lcg_prev(state):
    """The LCG step inverted (the multiplier is odd, so it has an inverse mod 2^32)."""
    return ((state - 12345) * pow(1103515245, -1, 1 << 32)) & M32


# ----------------------------------------------------------------------------- matrices, camera
def mat_identity(n=4):
    return [[F(1.0 if i == j else 0.0) for j in range(n)] for i in range(n)]


def mat_mul(a, b):
    """Matrix::operator* (math.h:96-104): dot(row(i), rhs.col(j))."""
    n = len(a)
    return [[dot(a[i], [b[k][j] for k in range(n)]) for j in range(n)] for i in range(n)]


def mat_vec(m, v):
    """Matrix * Array (math.h:89-95)."""
    return tuple(dot(r, v) for r in m)


def m_translate(v):
    """Transform::translate (math.h:266-269)."""
    o, z = F(1.0), F(0.0)
    return [[o, z, z, F(v[0])], [z, o, z, F(v[1])], [z, z, o, F(v[2])], [z, z, z, o]]


def m_scale(s):
    """Transform::scale (math.h:270-273)."""
    o, z = F(1.0), F(0.0)
    return [[F(s[0]), z, z, z], [z, F(s[1]), z, z], [z, z, F(s[2]), z], [z, z, z, o]]


def m_rotate_x(t):
    """math.h:274-279."""
    s, c, o, z = fsin(t), fcos(t), F(1.0), F(0.0)
    return [[o, z, z, z], [z, c, F(-s), z], [z, s, c, z], [z, z, z, o]]


def m_rotate_y(t):
    """math.h:281-286."""
    s, c, o, z = fsin(t), fcos(t), F(1.0), F(0.0)
    return [[c, z, s, z], [z, o, z, z], [F(-s), z, c, z], [z, z, z, o]]


def m_rotate_z(t):
    """math.h:288-293."""
    s, c, o, z = fsin(t), fcos(t), F(1.0), F(0.0)
    return [[c, F(-s), z, z], [s, c, z, z], [z, z, o, z], [z, z, z, o]]


def apply_point(m, p):
    """Transform::apply_point (math.h:243-251)."""
    v = mat_vec(m, (p[0], p[1], p[2], F(1.0)))
    q = v[:3]
    if v[3] != F(1.0):
        q = divs(q, v[3])
    return q


def apply_vector(m, v):
    """Transform::apply_vector (math.h:253): the upper-left 3x3 (math.h:234-239) times v."""
    return tuple(dot(m[i][:3], v) for i in range(3))


def radians32(x):
    """radians<float> (math.h:352-354): x * Pi / 180.0f."""
    return F(F(F(x) * PI) / F(180.0))


def radians64(x):
    """radians<double> (math.h:352-354): Constants<double>::Pi() is the f32 literal widened."""
    return float(x) * float(PI) / 180.0


class Camera:
    """PerspectiveCameraNode::compile (core/nodes/camera.cpp:32-39, 42-47) and
    PerspectiveCamera (kernel/camera.h:45-86).  position f32, rotation and fov in degrees as the
    scene file gives them (rotation f32, fov f64)."""

    def __init__(self, position, rotation_deg, fov_deg, resolution):
        rot = [radians32(F(r)) for r in rotation_deg]
        c2w = m_rotate_z(rot[2])
        c2w = mat_mul(m_rotate_x(rot[1]), c2w)
        c2w = mat_mul(m_rotate_y(rot[0]), c2w)
        c2w = mat_mul(m_translate(vec(position)), c2w)
        self.c2w = c2w
        self.res = (int(resolution[0]), int(resolution[1]))
        self.fov = F(radians64(fov_deg))                 # the kernel camera takes a Float
        rx, ry = self.res
        m = mat_identity()
        m = mat_mul(m_scale((F(F(1.0) / F(rx)), F(F(1.0) / F(ry)), F(1.0))), m)
        m = mat_mul(m_scale((2, 2, 1)), m)
        m = mat_mul(m_translate((-1, -1, 0)), m)
        m = mat_mul(m_scale((1, -1, 1)), m)
        s = fatan(F(self.fov / F(2.0)))
        if rx > ry:
            m = mat_mul(m_scale((s, F(F(s * F(ry)) / F(rx)), 1)), m)
        else:
            m = mat_mul(m_scale((F(F(s * F(rx)) / F(ry)), s, 1)), m)
        self.r2c = m

    def generate_ray(self, u1, u2, raster):
        """camera.h:67-86 with lens_radius 0 (the node never sets it): the lens draw is unused."""
        pf = (F(F(raster[0]) + u2[0]), F(F(raster[1]) + u2[1]))
        p = apply_point(self.r2c, (pf[0], pf[1], F(0.0)))
        d = normalize(sub((p[0], p[1], F(0.0)), (F(0.0), F(0.0), F(1.0))))
        o = apply_point(self.c2w, (F(0.0), F(0.0), F(0.0)))
        d = apply_vector(self.c2w, d)
        return o, d


# ----------------------------------------------------------------------------- warps
def concentric_disk(u):
    """kernel/sampling.h:32-46."""
    ox = F(F(F(2.0) * u[0]) - F(1.0))
    oy = F(F(F(2.0) * u[1]) - F(1.0))
    if ox == 0 and oy == 0:
        return (F(0.0), F(0.0))
    if fabs(ox) > fabs(oy):
        r = ox
        theta = F(PI4 * F(oy / ox))
    else:
        r = oy
        theta = F(PI2 - F(PI4 * F(ox / oy)))
    return (F(r * fcos(theta)), F(r * fsin(theta)))


def cosine_hemisphere(u):
    """sampling.h:48-53."""
    uv = concentric_disk(u)
    r = dot(uv, uv)
    h = fsqrt(std_max(F(0.0), F(F(1.0) - r)))
    return (uv[0], h, uv[1])


def cosine_hemisphere_pdf(cos_theta):
    """sampling.h:54-56."""
    return F(cos_theta * INV_PI)


def uniform_sample_triangle(u):
    """sampling.h:64-69."""
    su0 = fsqrt(u[0])
    return (F(F(1.0) - su0), F(u[1] * su0))


# ----------------------------------------------------------------------------- Frame
class Frame:
    """common/math.h:201-225."""

    def __init__(self, n):
        self.n = n
        if fabs(n[0]) > fabs(n[1]):
            self.T = divs((F(-n[2]), F(0.0), n[0]), fsqrt(F(F(n[0] * n[0]) + F(n[2] * n[2]))))
        else:
            self.T = divs((F(0.0), n[2], F(-n[1])), fsqrt(F(F(n[1] * n[1]) + F(n[2] * n[2]))))
        self.B = normalize(cross(n, self.T))

    def world_to_local(self, v):
        return (dot(self.T, v), dot(self.n, v), dot(self.B, v))

    def local_to_world(self, v):
        return add(add(scale(v[0], self.T), scale(v[1], self.n)), scale(v[2], self.B))


# ----------------------------------------------------------------------------- bsdf-funcs, GGX
def same_hemisphere(wo, wi):
    """kernel/bsdf-funcs.h:54-56."""
    return F(wo[1] * wi[1]) >= 0


def cos2_theta(w):
    """bsdf-funcs.h:32."""
    return F(w[1] * w[1])


def tan2_theta(w):
    """bsdf-funcs.h:34, 38: (1 - cos2) / cos2."""
    c2 = cos2_theta(w)
    return F(F(F(1.0) - c2) / c2)


def reflect(w, n):
    """bsdf-funcs.h:58-60: -1 * w + 2 * dot(w, n) * n."""
    return add(scale(F(-1.0), w), scale(F(F(2.0) * dot(w, n)), n))


def ggx_d(alpha, m):
    """kernel/microfacet.h:74-82."""
    if m[1] <= 0:
        return F(0.0)
    a2 = F(alpha * alpha)
    c2 = cos2_theta(m)
    t2 = tan2_theta(m)
    at = F(a2 + t2)
    return F(a2 / F(F(F(F(PI * c2) * c2) * at) * at))


def ggx_g1(alpha, v, m):
    """microfacet.h:84-89.  The literals are doubles, so the f32 product alpha * alpha * tan2(m)
    is widened and the rest runs in f64; the Float return rounds once."""
    if F(dot(v, m) * v[1]) <= 0:
        return F(0.0)
    x = float(F(F(alpha * alpha) * tan2_theta(m)))
    return F(2.0 / (1.0 + float(np.sqrt(np.float64(1.0 + x)))))


def ggx_g(alpha, i, o, m):
    """microfacet.h:122-124."""
    return F(ggx_g1(alpha, i, m) * ggx_g1(alpha, o, m))


def ggx_pdf(alpha, wh):
    """MicrofacetModel::evaluate_pdf (microfacet.h:150-152)."""
    return F(ggx_d(alpha, wh) * fabs(wh[1]))


def ggx_sample_wh(alpha, wo, u, count=None):
    """microfacet.h:125-149, the EGGX case."""
    phi = F(F(F(2.0) * PI) * u[1])
    t2 = F(F(F(alpha * alpha) * u[0]) / F(F(1.0) - u[0]))
    cos_t = F(F(1.0) / fsqrt(F(F(1.0) + t2)))
    sin_t = fsqrt(std_max(F(0.0), F(F(1.0) - F(cos_t * cos_t))))
    wh = (F(fcos(phi) * sin_t), cos_t, F(fsin(phi) * sin_t))
    flip = not same_hemisphere(wo, wh)
    if count is not None:
        count["sample_wh.flip" if flip else "sample_wh.keep"] += 1
    if flip:
        wh = neg(wh)
    return wh


# ----------------------------------------------------------------------------- closures
def diffuse_evaluate(R, wo, wi):
    """DiffuseBSDF::evaluate (kernel/material.h:69-74)."""
    if same_hemisphere(wo, wi):
        return scale(INV_PI, R)
    return (F(0.0),) * 3


def diffuse_sample(R, u, wo, count=None):
    """DiffuseBSDF::sample (material.h:76-85) -> (f, wi, pdf)."""
    wi = cosine_hemisphere(u)
    flip = not same_hemisphere(wo, wi)
    if count is not None:
        count["diffuse.flip" if flip else "diffuse.keep"] += 1
    if flip:
        wi = (wi[0], F(-wi[1]), wi[2])
    pdf = cosine_hemisphere_pdf(fabs(wi[1]))
    return scale(INV_PI, R), wi, pdf


def glossy_evaluate(R, alpha, wo, wi, count=None):
    """MicrofacetReflection::evaluate (material.h:103-120)."""
    def tick(k):
        if count is not None:
            count["glossy_eval." + k] += 1
    if not same_hemisphere(wo, wi):
        tick("other_side")
        return (F(0.0),) * 3
    cos_o = fabs(wo[1])
    cos_i = fabs(wi[1])
    wh = add(wo, wi)
    if cos_i == 0 or cos_o == 0:
        tick("grazing_zero")
        return (F(0.0),) * 3
    if wh[0] == 0 and wh[1] == 0 and wh[2] == 0:
        tick("wh_zero")
        return (F(0.0),) * 3
    wh = normalize(wh)
    if wh[1] < 0:
        tick("wh_flip")
        wh = neg(wh)
    else:
        tick("wh_keep")
    fr = F(1.0)
    s = F(F(F(ggx_d(alpha, wh) * ggx_g(alpha, wo, wi, wh)) * fr) / F(F(F(4.0) * cos_i) * cos_o))
    return scale(s, R)


def glossy_sample(R, alpha, u, wo, count=None):
    """MicrofacetReflection::sample (material.h:122-137) -> (f, wi, pdf)."""
    wh = ggx_sample_wh(alpha, wo, u, count)
    wi = reflect(wo, wh)
    if not same_hemisphere(wo, wi):
        if count is not None:
            count["glossy.other_side"] += 1
        return (F(0.0),) * 3, wi, F(0.0)
    if count is not None:
        count["glossy.same_side"] += 1
        count["glossy.wh_flip" if wh[1] < 0 else "glossy.wh_keep"] += 1
    if wh[1] < 0:
        wh = neg(wh)
    pdf = F(ggx_pdf(alpha, wh) / F(F(4.0) * fabs(dot(wo, wh))))
    return glossy_evaluate(R, alpha, wo, wi, count), wi, pdf


class BSDF:
    """BSDF (material.h:157-191): closure = ("diffuse", R) or ("glossy", R, alpha)."""

    def __init__(self, ng, ns, closure, choice_pdf=F(1.0)):
        self.ng, self.ns = ng, ns
        self.frame = Frame(ns)
        self.closure = closure
        self.choice_pdf = choice_pdf

    def evaluate(self, wo, wi, count=None):
        wo, wi = self.frame.world_to_local(wo), self.frame.world_to_local(wi)
        if self.closure[0] == "diffuse":
            return diffuse_evaluate(self.closure[1], wo, wi)
        return glossy_evaluate(self.closure[1], self.closure[2], wo, wi, count)

    def sample(self, u, wo, count=None):
        """-> (f, wi world, pdf * choice_pdf)."""
        wo = self.frame.world_to_local(wo)
        if self.closure[0] == "diffuse":
            f, wi, pdf = diffuse_sample(self.closure[1], u, wo, count)
        else:
            f, wi, pdf = glossy_sample(self.closure[1], self.closure[2], u, wo, count)
        return f, self.frame.local_to_world(wi), F(pdf * self.choice_pdf)


# ----------------------------------------------------------------------------- textures
def image_lookup(img, tc):
    """TImage::View::operator()(float2) then (int, int) (core/image.hpp:83-99): truncate
    p * resolution towards zero, clamp to the image.  img is float32 [h, w, 4]."""
    h, w = img.shape[0], img.shape[1]
    x = int(F(tc[0] * F(w)))
    y = int(F(tc[1] * F(h)))
    x = min(max(x, 0), w - 1)
    y = min(max(y, 0), h - 1)
    return vec(img[y, x, :3])


def texture_evaluate(tex, tc):
    """ConstantTexture / ImageTexture::evaluate (kernel/texture.h:35, 45-49).  tex is
    ("const", rgb) or ("image", array)."""
    if tex[0] == "const":
        return vec(tex[1])
    tx = F(math.fmod(float(tc[0]), 1.0))
    ty = F(math.fmod(float(tc[1]), 1.0))
    ty = F(F(1.0) - ty)
    return image_lookup(tex[1], (tx, ty))


def texture_integral(tex):
    """Texture::integral (texture.h:36, 50-56; luminance common/color.h:53-56)."""
    luma = (F(0.2126), F(0.7152), F(0.0722))
    if tex[0] == "const":
        return dot(vec(tex[1]), luma)
    img = tex[1]
    total = F(0.0)
    for px in img.reshape(-1, img.shape[-1]):
        total = F(total + dot(vec(px[:3]), luma))
    return F(total / F(img.shape[0] * img.shape[1]))


# ----------------------------------------------------------------------------- materials
# ("diffuse", color) ("glossy", color, roughness) ("emissive", color, double_sided)
# ("mix", fraction, A, B); None is a triangle without a material.
def select_material(mat, u, tc, count=None):
    """Material::select_material (material.h:255-271) -> (material, choice_pdf, u)."""
    choice = F(1.0)
    while mat is not None and mat[0] == "mix":
        frac = texture_evaluate(mat[1], tc)[0]
        if u < frac:
            u = F(u / frac)
            mat = mat[3]
            choice = F(choice * F(F(1.0) / frac))
            if count is not None:
                count["mix.B"] += 1
        else:
            u = F(F(u - frac) / F(F(1.0) - frac))
            mat = mat[2]
            choice = F(choice * F(F(1.0) / F(F(1.0) - frac)))
            if count is not None:
                count["mix.A"] += 1
    return mat, choice, u


def get_bsdf(mat, u1x, tc, ng, ns, count=None):
    """Material::get_bsdf (material.h:292-297) with get_bsdf0 (274-282) and the two materials'
    get_bsdf (210-215, 223-230).  None when the resolved material has no closure."""
    m, choice, _ = select_material(mat, u1x, tc, count)
    if m is None or m[0] in ("emissive", "mix"):
        return None
    R = texture_evaluate(m[1], tc)
    if m[0] == "diffuse":
        return BSDF(ng, ns, ("diffuse", R), choice)
    r = texture_evaluate(m[2], tc)[0]
    r = F(r * r)
    return BSDF(ng, ns, ("glossy", R, r), choice)


# ----------------------------------------------------------------------------- triangles, lights
class Triangle:
    """Triangle (kernel/shape.h:26-43) filled by get_triangle (kernel/instance.h:83-97)."""

    def __init__(self, v, n, t, material):
        self.v, self.n, self.t, self.material = v, n, t, material

    def p(self, uv):
        return lerp3(self.v[0], self.v[1], self.v[2], uv)

    def area(self):
        return F(length(cross(sub(self.v[1], self.v[0]), sub(self.v[2], self.v[0]))) * F(0.5))

    def ng(self):
        return normalize(cross(sub(self.v[1], self.v[0]), sub(self.v[2], self.v[0])))

    def ns(self, uv):
        return lerp3(self.n[0], self.n[1], self.n[2], uv)

    def texcoord(self, uv):
        return lerp3(self.t[0], self.t[1], self.t[2], uv)


def light_sample(tri, color, u, p_ref):
    """AreaLight::sample (kernel/light.h:58-71) -> dict(wi, pdf, L, ray o, d, tmin, tmax)."""
    coords = uniform_sample_triangle(u)
    p = tri.p(coords)
    ng = tri.ng()
    wi = sub(p, p_ref)
    d2 = dot(wi, wi)
    wi = divs(wi, fsqrt(d2))
    L = texture_evaluate(color, tri.texcoord(coords))
    pdf = F(F(d2 / std_max(F(0.0), F(-dot(wi, ng)))) / tri.area())
    tmin = F(EPS / fabs(dot(wi, ng)))
    tmax = F(fsqrt(d2) * F(F(1.0) - SHADOW_EPS))
    return dict(wi=wi, pdf=pdf, L=L, o=p, d=neg(wi), tmin=tmin, tmax=tmax)


class Distribution1D:
    """common/distribution.h:32-102 (the statement of tests/golden/make_golden.py's dist)."""

    def __init__(self, func):
        n = len(func)
        self.func = [F(x) for x in func]
        cdf = [F(0.0)] * (n + 1)
        for i in range(n):
            cdf[i + 1] = F(cdf[i] + F(self.func[i] / F(n)))
        self.func_int = cdf[n]
        if self.func_int == 0:
            cdf = [F(0.0)] + [F(F(i) / F(n)) for i in range(1, n + 1)]
        else:
            cdf = [cdf[0]] + [F(c / self.func_int) for c in cdf[1:]]
        self.cdf = cdf

    def sample_discrete(self, u):
        n = len(self.func)
        lo, hi = 0, n + 1
        while lo < hi:
            mid = (lo + hi) // 2
            if self.cdf[mid] <= u:
                lo = mid + 1
            else:
                hi = mid
        i = min(max(hi - 1, 0), n - 1)
        return i, F(self.func[i] / F(self.func_int * F(n)))


# ----------------------------------------------------------------------------- scene
def _tex(t):
    if t is None:
        return None
    if hasattr(t, "value"):
        return ("const", vec(t.value))
    return ("image", np.ascontiguousarray(t.image, np.float32))


def _mat(m, memo):
    if m is None:
        return None
    if id(m) in memo:
        return memo[id(m)]
    name = type(m).__name__
    if name == "DiffuseMaterial":
        r = ("diffuse", _tex(m.color))
    elif name == "GlossyMaterial":
        r = ("glossy", _tex(m.color), _tex(m.roughness))
    elif name == "EmissiveMaterial":
        r = ("emissive", _tex(m.color), bool(m.double_sided))
    elif name == "MixMaterial":
        r = ("mix", _tex(m.fraction), _mat(m.first, memo), _mat(m.second, memo))
    else:
        raise TypeError(name)
    memo[id(m)] = r
    return r


class RefScene:
    """SceneNode::compile (core/nodes/scene.cpp:43-95) from the scene description: raw mesh
    arrays and material objects.  Triangles are numbered mesh after mesh (global id)."""

    def __init__(self, scene):
        cam = scene.camera
        self.camera = Camera(cam.position, cam.rotation, cam.fov, cam.resolution)
        self.tris = []
        memo = {}
        for mesh in scene.shapes:
            v = np.asarray(mesh.vertices, np.float32).reshape(-1, 3)
            idx = np.asarray(mesh.indices, np.int32).reshape(-1, 3)
            nrm = np.asarray(mesh.normals, np.float32).reshape(-1, 3, 3)
            tcs = np.asarray(mesh.texcoords, np.float32).reshape(-1, 3, 2)
            mi = np.asarray(mesh.material_indices, np.int32)
            mats = [_mat(m, memo) for m in mesh.materials]
            for prim in range(idx.shape[0]):
                # Scene::get_triangle (kernel/scene.h:70-78): index -1 leaves the material null
                m = mats[mi[prim]] if mi[prim] != -1 else None
                self.tris.append(Triangle([vec(v[idx[prim, k]]) for k in range(3)],
                                          [vec(nrm[prim, k]) for k in range(3)],
                                          [vec(tcs[prim, k]) for k in range(3)], m))
        # light list and power (scene.cpp:51-88); tc_area and the product run in double
        self.lights, power = [], []
        for gid, tri in enumerate(self.tris):
            m = tri.material
            if m is None or m[0] != "emissive":
                continue
            integral = texture_integral(m[1])
            tc = [(t[0], t[1], F(0.0)) for t in tri.t]
            tc_area = float(length(cross(sub(tc[1], tc[0]), sub(tc[2], tc[0])))) * 0.5
            area = length(cross(sub(tri.v[1], tri.v[0]), sub(tri.v[2], tri.v[0])))
            power.append(F(float(area) * tc_area * float(integral)))
            self.lights.append(gid)
        self.power = power
        self.dist = Distribution1D(power) if power else None
        # exact duplicates (the Cornell fixture lists two of its triangles twice): same vertices,
        # normals, texcoords and material, so a tie between them changes nothing but the id
        self.canon, seen = [], {}
        for gid, t in enumerate(self.tris):
            key = (tuple(map(tuple, t.v)), tuple(map(tuple, t.n)), tuple(map(tuple, t.t)), id(t.material))
            self.canon.append(seen.setdefault(key, gid))
        # arrays for the brute-force intersection
        self.V0 = np.array([t.v[0] for t in self.tris], np.float32)
        self.E1 = (np.array([t.v[1] for t in self.tris], np.float32) - self.V0).astype(np.float32)
        self.E2 = (np.array([t.v[2] for t in self.tris], np.float32) - self.V0).astype(np.float32)

    def select_light(self, u):
        """Scene::select_light (kernel/scene.h:79-90) -> (global triangle id or None, pdf)."""
        if not self.lights:
            return None, F(0.0)
        i, pdf = self.dist.sample_discrete(u[0])
        if i == len(self.lights):
            i -= 1
        return self.lights[i], pdf


def _dot_rows(a, b):
    s = (a[:, 0] * b[:, 0]).astype(np.float32)
    s = (s + (a[:, 1] * b[:, 1]).astype(np.float32)).astype(np.float32)
    return (s + (a[:, 2] * b[:, 2]).astype(np.float32)).astype(np.float32)


def _cross_rows(a, b):
    x = (a[:, 1] * b[:, 2]).astype(np.float32) - (a[:, 2] * b[:, 1]).astype(np.float32)
    y = (a[:, 2] * b[:, 0]).astype(np.float32) - (a[:, 0] * b[:, 2]).astype(np.float32)
    z = (a[:, 0] * b[:, 1]).astype(np.float32) - (a[:, 1] * b[:, 0]).astype(np.float32)
    return np.stack([x, y, z], axis=1).astype(np.float32)


def intersect_all(sc, o, d, tmin, tmax):
    """MeshInstance::intersect (kernel/instance.h:42-80) for every triangle at once, the same f32
    operations per triangle -> (accepted mask, t, u, v), before the closest-hit comparison."""
    n = sc.V0.shape[0]
    D = np.broadcast_to(np.array(d, np.float32), (n, 3))
    O = np.broadcast_to(np.array(o, np.float32), (n, 3))
    h = _cross_rows(D, sc.E2)
    a = _dot_rows(sc.E1, h)
    ok = ~((a > F(-1e-6)) & (a < F(1e-6)))
    f = (F(1.0) / a).astype(np.float32)
    s = (O - sc.V0).astype(np.float32)
    u = (f * _dot_rows(s, h)).astype(np.float32)
    ok &= ~((u < 0.0) | (u > 1.0))
    q = _cross_rows(s, sc.E1)
    v = (f * _dot_rows(D, q)).astype(np.float32)
    ok &= ~((v < 0.0) | ((u + v).astype(np.float32) > 1.0))
    t = (f * _dot_rows(sc.E2, q)).astype(np.float32)
    ok &= (t > F(tmin)) & (t < F(tmax))
    return ok, t, u, v


class Tracer:
    """Scene::intersect / occlude as a loop over all triangles in global order (the leaf test of
    kernel/bvh-accelerator.h:476-486 keeps the first of equal t: instance.h:68)."""

    def __init__(self, sc):
        self.sc = sc
        self.ambiguous = False
        self.closest = 0
        self.shadow = 0

    def _flag(self, d):
        if d[0] == 0 or d[1] == 0 or d[2] == 0:
            self.ambiguous = True

    def intersect(self, o, d, tmin, tmax):
        self._flag(d)
        ok, t, u, v = intersect_all(self.sc, o, d, tmin, tmax)
        if not ok.any():
            return None
        tt = np.where(ok, t, np.float32(np.inf))
        gid = int(np.argmin(tt))            # first index of the minimum: strict t < hit->t
        if any(self.sc.canon[i] != self.sc.canon[gid] for i in np.nonzero(tt == tt[gid])[0]):
            self.ambiguous = True
        return gid, F(t[gid]), F(u[gid]), F(v[gid])

    def occlude(self, o, d, tmin, tmax):
        self._flag(d)
        ok, _, _, _ = intersect_all(self.sc, o, d, tmin, tmax)
        return bool(ok.any())


# ----------------------------------------------------------------------------- path tracer
def is_black(c):
    """Color::is_black (common/color.h:48-50) through reduce (common/array.h:217-224): the
    accumulator starts as c[0] itself, so the first channel counts when it is non-zero (negative
    and NaN included), the other two when they are > 0."""
    return not (bool(c[0] != 0) or c[1] > 0 or c[2] > 0)


def path_sample(sc, sampler, px, py, max_depth, count=None, tracer=None, record=None, roles=None):
    """GenericPathTracer::run_megakernel (kernel/pathtracer.h:133-164) with camera_ray (61-64),
    select_light (65-67), compute_direct_lighting (69-91) and on_surface_scatter (96-132).
    Returns L; `sampler` advances as pt.sampler does.  tracer.closest counts the scene.intersect
    calls made while depth < max(1, max_depth): a later call can change neither L nor the
    sampler (on_surface_scatter adds only at depth 0 and scatters only below max_depth).
    `roles` collects (name, value) of the draws the edge-pixel search aims at."""
    def tick(k):
        if count is not None:
            count[k] += 1
    tr = tracer if tracer is not None else Tracer(sc)
    L = (F(0.0),) * 3
    beta = (F(1.0),) * 3
    depth = 0
    u1 = sampler.next2d()
    u2 = sampler.next2d()
    o, d = sc.camera.generate_ray(u1, u2, (px, py))
    tmin, tmax = EPS, INF
    if record is not None:
        record["o"], record["d"] = o, d
    first = True
    while True:
        if depth < max(1, max_depth):
            tr.closest += 1
        hit = tr.intersect(o, d, tmin, tmax)
        if first and record is not None:
            record["hit"] = hit
        first = False
        if hit is None:
            tick("miss")
            break
        gid, _, hu, hv = hit
        uv = (hu, hv)
        tri = sc.tris[gid]
        wo = neg(d)
        p, ng, ns, tc = tri.p(uv), tri.ng(), tri.ns(uv), tri.texcoord(uv)
        mat = tri.material
        # MaterialEvalContext (material.h:198-202) takes the sampler by value: its four draws
        # come from a copy, pt.sampler does not advance
        ctx = sampler.copy()
        cu1 = ctx.next2d()
        ctx.next2d()
        if mat is None:
            tick("scatter.null_material")
            break
        if mat[0] == "emissive":
            if depth == 0:
                front = dot(neg(wo), ng) < 0
                if mat[2] or front:
                    tick("scatter.emit_double" if mat[2] else "scatter.emit_front")
                    L = add(L, mul(beta, texture_evaluate(mat[1], tc)))
                else:
                    tick("scatter.emit_back")
            else:
                tick("scatter.emissive_deep")
            break
        if not depth < max_depth:
            tick("scatter.max_depth")
            break
        if roles is not None and mat[0] == "mix":
            roles.append(("mix_u_at_frac", F(cu1[0] == texture_evaluate(mat[1], tc)[0])))
        bsdf = get_bsdf(mat, cu1[0], tc, ng, ns, count)
        # pathtracer.h:120 draws the BSDF sample before :121 uses the closure, so a Mix that
        # resolved to Emissive (no closure) ends the path after that draw
        su = sampler.next2d()
        if bsdf is None:
            tick("scatter.mix_to_emissive")
            break
        if roles is not None and bsdf.closure[0] == "glossy":
            roles.append(("ggx_ux", su[0]))
        f, wi, pdf = bsdf.sample(su, wo, count)
        if pdf == 0:
            tick("scatter.pdf_zero")
            break
        tick("scatter.event")
        cosg = fabs(dot(ng, wi))
        ev_tmin = F(EPS / cosg)
        ev_beta = divs(scale(cosg, f), pdf)
        # direct lighting (pathtracer.h:151-158)
        sel_u = sampler.next2d()
        lid, lpdf = sc.select_light(sel_u)
        if lid is not None:
            ltri = sc.tris[lid]
            lu = sampler.next2d()
            if roles is not None:
                roles += [("light_select", sel_u[0]), ("light_ux", lu[0]), ("light_uy", lu[1])]
            ls = light_sample(ltri, ltri.material[1], lu, p)
            if ls["pdf"] <= 0:
                tick("direct.pdf_nonpositive")
            else:
                lpdf = F(lpdf * ls["pdf"])
                fl = scale(fabs(dot(ns, ls["wi"])), mul(ls["L"], bsdf.evaluate(wo, ls["wi"], count)))
                color = divs(mul(beta, fl), lpdf)
                if is_black(color):
                    tick("direct.black")
                else:
                    tr.shadow += 1
                    if tr.occlude(ls["o"], ls["d"], ls["tmin"], ls["tmax"]):
                        tick("direct.occluded")
                    else:
                        tick("direct.lit")
                        L = add(L, color)
        else:
            tick("direct.no_light")
        beta = mul(beta, ev_beta)
        depth += 1
        o, d, tmin, tmax = p, wi, ev_tmin, INF
    return L


def clamp_radiance(L, ray_clamp):
    """The GPU integrator's splat (kernel/integrators/gpu/cuda/integrator.cpp:397-398) with
    Color::clamp_zero (common/color.h:35-47); applied only when ray_clamp > 0."""
    out = []
    for x in L:
        x = F(0.0) if np.isnan(x) else std_max(F(0.0), x)
        out.append(std_min(x, F(ray_clamp)))
    return tuple(out)


def render_pixel(sc, x, y, spp, max_depth, ray_clamp=0.0, count=None, width=None, roles=None):
    """One pixel of cpu::PathTracer::render's loop (kernel/integrators/cpu/integrator.cpp:
    115-137): the sampler is seeded with x + y * width and runs on through the pixel's samples;
    the tile adds each sample's L with weight 1 (core/film.h:66-70).
    -> dict(radiance, weight, seed, closest, shadow, ambiguous, first=sample 0's ray and hit)."""
    w = sc.camera.res[0] if width is None else width
    sampler = LCG((x + y * w) & M32)
    rad = (F(0.0),) * 3
    weight = F(0.0)
    tr = Tracer(sc)
    first = {}
    for s in range(spp):
        rec = first if s == 0 else None
        L = path_sample(sc, sampler, x, y, max_depth, count, tr, rec, roles)
        if ray_clamp > 0:
            L = clamp_radiance(L, ray_clamp)
        weight = F(weight + F(1.0))
        rad = add(rad, L)
    return dict(radiance=rad, weight=weight, seed=sampler.seed, closest=tr.closest, shadow=tr.shadow,
                ambiguous=tr.ambiguous, first=first)


def new_counts():
    return Counter()

"""The environment light restated in numpy f32 on top of ref_restate.py.

The reference has no environment light (a ray that leaves the scene adds nothing, pathtracer.h:93), so
this file is the definition's second statement rather than a second reading: the octahedral map, its
piecewise-constant distribution built with the reference's Distribution1D, and the path loop of
ref_restate.path_sample with the two additions (the depth-0 miss, the environment's branch of direct
lighting).  One f32 operation per operation of the definition, left to right; only add, multiply,
divide, sqrt, abs and compare occur.  It shares no code with the HIP library.
"""
import numpy as np

import ref_restate as R
from ref_restate import EPS, F, INF, add, divs, dot, fabs, fsqrt, mul, neg, scale

LUMA = (F(0.2126), F(0.7152), F(0.0722))     # Color::luminance, common/color.h:52-55
ONE, TWO, HALF, QUARTER = F(1.0), F(2.0), F(0.5), F(0.25)


def sgn(x):
    """sgn 0 = +1 (and so is sgn -0)."""
    return F(-1.0) if x < 0 else ONE


def fold(x, y):
    """The lower hemisphere's half of the square: its corners folded over |x| + |y| = 1."""
    return F(F(ONE - fabs(y)) * sgn(x)), F(F(ONE - fabs(x)) * sgn(y))


def decode(x, y):
    """Point of [-1, 1]^2 -> (unit direction in map space, |q|_2 of the octahedron's point q)."""
    x, y = F(x), F(y)
    z = F(F(ONE - fabs(x)) - fabs(y))
    if z < 0:
        x, y = fold(x, y)
    q = (x, y, z)
    ln = fsqrt(dot(q, q))
    return divs(q, ln), ln


def texel_of(x, n):
    i = int(F(F(F(x * HALF) + HALF) * F(n)))
    return min(max(i, 0), n - 1)


def encode(d, n):
    """Direction in map space -> (i, j, |q|_2)."""
    l1 = F(F(fabs(d[0]) + fabs(d[1])) + fabs(d[2]))
    q = divs(d, l1)
    ln = fsqrt(dot(q, q))
    x, y = q[0], q[1]
    if q[2] < 0:
        x, y = fold(x, y)
    return texel_of(x, n), texel_of(y, n), ln


def texel_point(k, offset, n):
    """Coordinate of the point `offset` in [0, 1] across texel k."""
    return F(F(F(F(F(k) + F(offset)) / F(n)) * TWO) - ONE)


class Dist(R.Distribution1D):
    """Distribution1D with the in-interval remap of a draw and a pdf of 0 for a function that is 0
    everywhere (no draw selects it; func / (0 * n) would be NaN)."""

    def pdf(self, i):
        if self.func_int == 0:
            return F(0.0)
        return F(self.func[i] / F(self.func_int * F(len(self.func))))

    def sample(self, u):
        i, _ = self.sample_discrete(u)
        off = F(F(u - self.cdf[i]) / F(self.cdf[i + 1] - self.cdf[i]))
        return i, off, self.pdf(i)


class Environment:
    def __init__(self, rgb, scale3=(1.0, 1.0, 1.0), select_prob=0.5, world_to_env=None):
        self.map = np.ascontiguousarray(rgb, np.float32)
        n = self.map.shape[0]
        assert self.map.shape == (n, n, 3) and n >= 1
        self.n = n
        self.scale = R.vec(scale3)
        self.select_prob = F(select_prob)
        self.R = [F(v) for v in (np.eye(3).reshape(-1) if world_to_env is None else np.reshape(world_to_env, -1))]
        self.rows = []
        for j in range(n):
            yc = texel_point(j, 0.5, n)
            func = []
            for i in range(n):
                _, ln = decode(texel_point(i, 0.5, n), yc)
                func.append(F(dot(self.lookup(i, j), LUMA) / F(F(ln * ln) * ln)))
            self.rows.append(Dist(func))
        self.marginal = Dist([r.func_int for r in self.rows])

    def lookup(self, i, j):
        """Texel (i, j) with the scale applied."""
        return mul(R.vec(self.map[j, i]), self.scale)

    def to_map(self, d):
        m = self.R
        return (dot(m[0:3], d), dot(m[3:6], d), dot(m[6:9], d))

    def to_world(self, d):
        m = self.R
        return (dot((m[0], m[3], m[6]), d), dot((m[1], m[4], m[7]), d), dot((m[2], m[5], m[8]), d))

    def pdf(self, i, j, ln):
        P = F(self.marginal.pdf(j) * self.rows[j].pdf(i))
        if not P > 0:       # a texel no draw selects: 0 whatever the point (whose offset may be 0 / 0)
            return F(0.0)
        fn = F(self.n)
        return F(F(P * F(F(fn * fn) * QUARTER)) * F(F(ln * ln) * ln))

    def sample(self, u):
        """u = (ux, uy) -> (world direction, radiance of the sampled texel, solid-angle pdf, (i, j))."""
        j, oy, _ = self.marginal.sample(u[1])
        i, ox, _ = self.rows[j].sample(u[0])
        d, ln = decode(texel_point(i, ox, self.n), texel_point(j, oy, self.n))
        return self.to_world(d), self.lookup(i, j), self.pdf(i, j, ln), (i, j)

    def eval(self, d_world):
        """World direction -> (radiance of the texel it looks up, pdf with which sampling draws it, (i, j))."""
        i, j, ln = encode(self.to_map(d_world), self.n)
        return self.lookup(i, j), self.pdf(i, j, ln), (i, j)


def path_sample(sc, env, sampler, px, py, max_depth, count=None, tracer=None, record=None, roles=None):
    """ref_restate.path_sample with an environment: a camera ray that misses adds beta * Le; direct
    lighting draws su and lu whenever there is any light, takes the environment when there is no area
    light or su.x < select_prob, and otherwise an area light from the remapped draw, its selection pdf
    times 1 - select_prob.  Everything else is path_sample's, statement for statement."""
    def tick(k):
        if count is not None:
            count[k] += 1
    tr = tracer if tracer is not None else R.Tracer(sc)
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
            if depth == 0:
                tick("miss.sky")
                Le, _, _ = env.eval(d)
                L = add(L, mul(beta, Le))
            else:
                tick("miss")
            break
        gid, _, hu, hv = hit
        uv = (hu, hv)
        tri = sc.tris[gid]
        wo = neg(d)
        p, ng, ns, tc = tri.p(uv), tri.ng(), tri.ns(uv), tri.texcoord(uv)
        mat = tri.material
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
                    tick("scatter.emit")
                    L = add(L, mul(beta, R.texture_evaluate(mat[1], tc)))
            break
        if not depth < max_depth:
            tick("scatter.max_depth")
            break
        bsdf = R.get_bsdf(mat, cu1[0], tc, ng, ns, count)
        su = sampler.next2d()
        if bsdf is None:
            break
        f, wi, pdf = bsdf.sample(su, wo, count)
        if pdf == 0:
            tick("scatter.pdf_zero")
            break
        tick("scatter.event")
        cosg = fabs(dot(ng, wi))
        ev_tmin = F(EPS / cosg)
        ev_beta = divs(scale(cosg, f), pdf)
        # direct lighting: one light of {environment, area lights}
        sel_u = sampler.next2d()
        lu = sampler.next2d()
        sp = env.select_prob
        if roles is not None:
            roles += [("light_select", sel_u[0]), ("light_ux", lu[0]), ("light_uy", lu[1])]
        if not sc.lights or sel_u[0] < sp:
            sel_pdf = sp if sc.lights else ONE
            if roles is not None:
                roles += [("env_ux", lu[0]), ("env_uy", lu[1])]
            ewi, Le, epdf, _ = env.sample(lu)
            if epdf <= 0:
                tick("env.pdf_nonpositive")
            else:
                fl = scale(fabs(dot(ns, ewi)), mul(Le, bsdf.evaluate(wo, ewi, count)))
                color = divs(mul(beta, fl), F(sel_pdf * epdf))
                if R.is_black(color):
                    tick("env.black")
                else:
                    tr.shadow += 1
                    if tr.occlude(p, ewi, F(EPS / fabs(dot(ng, ewi))), INF):
                        tick("env.occluded")
                    else:
                        tick("env.lit")
                        L = add(L, color)
        else:
            lid, lpdf = sc.select_light((F(F(sel_u[0] - sp) / F(ONE - sp)), sel_u[1]))
            lpdf = F(lpdf * F(ONE - sp))
            ltri = sc.tris[lid]
            ls = R.light_sample(ltri, ltri.material[1], lu, p)
            if ls["pdf"] <= 0:
                tick("direct.pdf_nonpositive")
            else:
                lpdf = F(lpdf * ls["pdf"])
                fl = scale(fabs(dot(ns, ls["wi"])), mul(ls["L"], bsdf.evaluate(wo, ls["wi"], count)))
                color = divs(mul(beta, fl), lpdf)
                if R.is_black(color):
                    tick("direct.black")
                else:
                    tr.shadow += 1
                    if tr.occlude(ls["o"], ls["d"], ls["tmin"], ls["tmax"]):
                        tick("direct.occluded")
                    else:
                        tick("direct.lit")
                        L = add(L, color)
        beta = mul(beta, ev_beta)
        depth += 1
        o, d, tmin, tmax = p, wi, ev_tmin, INF
    return L


def render_pixel(sc, env, x, y, spp, max_depth, ray_clamp=0.0, count=None, width=None, roles=None):
    """ref_restate.render_pixel under an environment."""
    w = sc.camera.res[0] if width is None else width
    sampler = R.LCG((x + y * w) & R.M32)
    rad = (F(0.0),) * 3
    weight = F(0.0)
    tr = R.Tracer(sc)
    first = {}
    for s in range(spp):
        rec = first if s == 0 else None
        L = path_sample(sc, env, sampler, x, y, max_depth, count, tr, rec, roles)
        if ray_clamp > 0:
            L = R.clamp_radiance(L, ray_clamp)
        weight = F(weight + F(1.0))
        rad = add(rad, L)
    return dict(radiance=rad, weight=weight, seed=sampler.seed, closest=tr.closest, shadow=tr.shadow,
                ambiguous=tr.ambiguous, first=first)

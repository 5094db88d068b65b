"""Mirror and Glass restated in numpy f32 on top of ref_restate.py, env_restate.py and
mis_restate.py.

The reference knows no material that reflects or refracts sharply, so this file is the definition, as
env_restate.py is the environment light's.  `path_sample` is mis_restate.path_sample statement for statement with
the additions marked `# SPEC`; on a scene without a Mirror or a Glass it computes what that one does.  All
arithmetic is f32, unfused, left to right, and uses only add, subtract, multiply, divide, sqrt, abs and compare,
so each step is the same IEEE operation in numpy, in host C++ and on the device.  It shares no code with the HIP
library.

The estimator.  A delta lobe evaluates to 0 for every direction next-event estimation can draw, so direct lighting
at such a vertex draws its numbers as at any other, finds the colour black and traces no shadow ray: no draw is
added, moved or removed.  The path carries one bit, via_delta: whether the closure its last scattering vertex
sampled (after Mix resolution) was a Mirror or a Glass.  An emitter, or the environment at a miss, that a ray
reaches via_delta counts at full weight, as it does for the camera ray, and the path ends there.  Found at
depth > 0 such a term is the path's terminal term E, added after everything else (mis_restate.py's order).

The ray at depth == max_depth.  The reference's loop still intersects it, and only the emission test precedes the
`depth >= max_depth` return; without a delta lobe that test cannot pass there, so the ray is neither traced nor
counted (ref_restate.path_sample).  Via a delta lobe it can, so exactly those rays are traced and counted.

There is no eta^2 radiance scaling: it cancels over a solid that is entered and left, and a camera inside a medium
is out of scope.  The refracted direction is not renormalised.
"""
import numpy as np

import env_restate as E
import mis_restate as M
import ref_restate as R
from ref_restate import EPS, F, INF, add, divs, dot, fabs, fsqrt, mul, neg, scale, sub

ZERO, ONE, HALF = F(0.0), F(1.0), F(0.5)
BLACK = (ZERO, ZERO, ZERO)


# ----------------------------------------------------------------------------- scene
def _mat(m, memo):
    """ref_restate._mat with ("mirror", color) and ("glass", color, ior)."""
    if m is None:
        return None
    if id(m) in memo:
        return memo[id(m)]
    name = type(m).__name__
    if name == "MirrorMaterial":
        r = ("mirror", R._tex(m.color))
    elif name == "GlassMaterial":
        r = ("glass", R._tex(m.color), F(m.ior))
    elif name == "MixMaterial":
        r = ("mix", R._tex(m.fraction), _mat(m.first, memo), _mat(m.second, memo))
    else:
        r = R._mat(m, {})
    memo[id(m)] = r
    return r


class SpecScene(R.RefScene):
    """RefScene over the six material types.  RefScene's own constructor refuses the two new ones, so the
    triangles' materials are built here and everything that follows from them is RefScene's, statement for
    statement (lights and their power, the duplicate map, the intersection arrays)."""

    def __init__(self, scene):
        cam = scene.camera
        self.camera = R.Camera(cam.position, cam.rotation, cam.fov, cam.resolution)
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
                m = mats[mi[prim]] if mi[prim] != -1 else None
                self.tris.append(R.Triangle([R.vec(v[idx[prim, k]]) for k in range(3)],
                                            [R.vec(nrm[prim, k]) for k in range(3)],
                                            [R.vec(tcs[prim, k]) for k in range(3)], m))
        self.lights, power = [], []
        for gid, tri in enumerate(self.tris):
            m = tri.material
            if m is None or m[0] != "emissive":
                continue
            integral = R.texture_integral(m[1])
            tc = [(t[0], t[1], F(0.0)) for t in tri.t]
            tc_area = float(R.length(R.cross(sub(tc[1], tc[0]), sub(tc[2], tc[0])))) * 0.5
            area = R.length(R.cross(sub(tri.v[1], tri.v[0]), sub(tri.v[2], tri.v[0])))
            power.append(F(float(area) * tc_area * float(integral)))
            self.lights.append(gid)
        self.power = power
        self.dist = R.Distribution1D(power) if power else None
        self.canon, seen = [], {}
        for gid, t in enumerate(self.tris):
            key = (tuple(map(tuple, t.v)), tuple(map(tuple, t.n)), tuple(map(tuple, t.t)), id(t.material))
            self.canon.append(seen.setdefault(key, gid))
        self.V0 = np.array([t.v[0] for t in self.tris], np.float32)
        self.E1 = (np.array([t.v[1] for t in self.tris], np.float32) - self.V0).astype(np.float32)
        self.E2 = (np.array([t.v[2] for t in self.tris], np.float32) - self.V0).astype(np.float32)


# ----------------------------------------------------------------------------- closures
def fresnel(c, ior, entering):
    """-> (F, ct, r) for the cosine c = |wo.y| > 0 of the incident side.  ct is None under total internal
    reflection (s2 >= 1), where F = 1 and nothing reads ct."""
    c, ior = F(c), F(ior)
    ei = ONE if entering else ior
    et = ior if entering else ONE
    r = F(ei / et)
    s2 = F(F(r * r) * R.std_max(ZERO, F(ONE - F(c * c))))
    if s2 >= ONE:
        return ONE, None, r
    ct = fsqrt(F(ONE - s2))
    rp = F(F(F(et * c) - F(ei * ct)) / F(F(et * c) + F(ei * ct)))
    rs = F(F(F(ei * c) - F(et * ct)) / F(F(ei * c) + F(et * ct)))
    return F(F(F(rp * rp) + F(rs * rs)) * HALF), ct, r


def mirror_sample(Rc, wo, count=None):
    """-> (f, wi, pdf) in the shading frame (y the normal)."""
    c = fabs(wo[1])
    if c == 0:
        if count is not None:
            count["delta.grazing"] += 1
        return BLACK, (F(-wo[0]), wo[1], F(-wo[2])), ZERO
    if count is not None:
        count["mirror.reflect"] += 1
    wi = (F(-wo[0]), wo[1], F(-wo[2]))
    return divs(Rc, fabs(wi[1])), wi, ONE


def glass_sample(Rc, ior, u, wo, count=None):
    """-> (f, wi, pdf).  The choice reads u[1]: under a Mix u[0] is the number that selected the material."""
    def tick(k):
        if count is not None:
            count[k] += 1
    c = fabs(wo[1])
    if c == 0:
        tick("delta.grazing")
        return BLACK, (F(-wo[0]), wo[1], F(-wo[2])), ZERO
    entering = bool(wo[1] > 0)
    Fr, ct, r = fresnel(c, ior, entering)
    if u[1] < Fr:
        tick("glass.tir" if ct is None else ("glass.reflect_outside" if entering else "glass.reflect_inside"))
        wi = (F(-wo[0]), wo[1], F(-wo[2]))
        return divs(scale(Fr, Rc), fabs(wi[1])), wi, Fr
    w = F(ONE - Fr)
    if ct is None:                     # u[1] == 1 under total internal reflection: pdf 0 ends the path
        tick("glass.tir_pdf_zero")
        return BLACK, (F(-wo[0]), wo[1], F(-wo[2])), w
    tick("glass.enter" if entering else "glass.leave")
    wi = (F(F(-r) * wo[0]), F(-ct) if entering else ct, F(F(-r) * wo[2]))
    return divs(scale(w, Rc), fabs(wi[1])), wi, w


def is_delta(closure):
    return closure[0] in ("mirror", "glass")


def get_bsdf(mat, u1x, tc, ng, ns, count=None):
    """ref_restate.get_bsdf with the two delta closures: ("mirror", R) and ("glass", R, ior)."""
    m, choice, _ = R.select_material(mat, u1x, tc, count)
    if m is not None and m[0] == "mirror":
        return R.BSDF(ng, ns, ("mirror", R.texture_evaluate(m[1], tc)), choice)
    if m is not None and m[0] == "glass":
        return R.BSDF(ng, ns, ("glass", R.texture_evaluate(m[1], tc), m[2]), choice)
    return _resolved_bsdf(m, choice, tc, ng, ns)


def _resolved_bsdf(m, choice, tc, ng, ns):
    """ref_restate.get_bsdf after its select_material, for a material this file has already resolved."""
    if m is None or m[0] in ("emissive", "mix"):
        return None
    Rc = R.texture_evaluate(m[1], tc)
    if m[0] == "diffuse":
        return R.BSDF(ng, ns, ("diffuse", Rc), choice)
    r = R.texture_evaluate(m[2], tc)[0]
    r = F(r * r)
    return R.BSDF(ng, ns, ("glossy", Rc, r), choice)


def bsdf_evaluate(bsdf, wo, wi, count=None):
    """0 for a delta closure, for every pair of directions."""
    if is_delta(bsdf.closure):
        return BLACK
    return bsdf.evaluate(wo, wi, count)


def closure_pdf(closure, wo, wi):
    return ZERO if is_delta(closure) else M.closure_pdf(closure, wo, wi)


# ----------------------------------------------------------------------------- path tracer
def path_sample(sc, sampler, px, py, max_depth, count=None, tracer=None, record=None, roles=None, env=None, mis=False):
    def tick(k):
        if count is not None:
            count[k] += 1
    tr = tracer if tracer is not None else R.Tracer(sc)
    if not hasattr(sc, "_mis_tri_sel"):
        sc._mis_tri_sel = M.tri_select_pdf(sc) if sc.lights else {}
    L = BLACK
    Eterm = BLACK                      # the terminal term: MIS's carried pair, or what a via_delta ray met
    carry = None
    via_delta = False                  # SPEC
    beta = (ONE,) * 3
    depth = 0
    u1 = sampler.next2d()
    u2 = sampler.next2d()
    o, d = sc.camera.generate_ray(u1, u2, (px, py))
    tmin, tmax = EPS, INF
    if record is not None:
        record["o"], record["d"] = o, d
    first = True
    while True:
        if depth < max(1, max_depth) or via_delta:             # SPEC: via_delta the ray at max_depth is traced
            tr.closest += 1
        hit = tr.intersect(o, d, tmin, tmax)
        if first and record is not None:
            record["hit"] = hit
        first = False
        if hit is None:
            if depth == 0 and env is not None:
                tick("miss.sky")
                Le, _, _ = env.eval(d)
                L = add(L, mul(beta, Le))
            elif via_delta and env is not None:                # SPEC: the sky seen in a mirror or through a pane
                tick("spec.miss_sky")
                Le, _, _ = env.eval(d)
                Eterm = mul(beta, Le)
            else:
                tick("miss")
                if carry is not None and env is not None:
                    T, p_b = carry
                    Le, p_w, _ = env.eval(d)
                    p_l = F((env.select_prob if sc.lights else ONE) * p_w)
                    if p_l > 0:
                        tick("mis.term_env")
                        Eterm = scale(M.power_weight(p_b, p_l), mul(T, Le))
                    else:
                        tick("mis.term_env_pdf_nonpositive")
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
            if depth == 0 or via_delta:                        # SPEC: the added term
                front = dot(neg(wo), ng) < 0
                if mat[2] or front:
                    e = mul(beta, R.texture_evaluate(mat[1], tc))
                    if depth == 0:
                        tick("scatter.emit")
                        L = add(L, e)
                    else:
                        tick("spec.emit_double" if mat[2] and not front else "spec.emit_front")
                        Eterm = e
                elif depth > 0:
                    tick("spec.emit_back")
            elif carry is not None:
                T, p_b = carry
                c = F(-dot(d, ng))
                po = sub(p, o)
                d2 = dot(po, po)
                sel = sc._mis_tri_sel.get(gid, F(0.0))
                if env is not None:
                    sel = F(sel * F(ONE - env.select_prob))
                p_l = F(sel * F(F(d2 / c) / tri.area()))
                if not c > 0:
                    tick("mis.term_area_back")
                elif not p_l > 0:
                    tick("mis.term_area_pdf_nonpositive")
                else:
                    tick("mis.term_area")
                    Eterm = scale(M.power_weight(p_b, p_l), mul(T, R.texture_evaluate(mat[1], tc)))
            break
        if not depth < max_depth:
            tick("scatter.max_depth")
            break
        through_mix = mat[0] == "mix"
        bsdf = get_bsdf(mat, cu1[0], tc, ng, ns, count)
        su = sampler.next2d()
        if bsdf is None:
            tick("scatter.mix_to_emissive")
            break
        delta = is_delta(bsdf.closure)                         # SPEC
        if delta and through_mix:
            tick("spec.delta_through_mix")
        last = not depth + 1 < max_depth
        pair = mis and not last and not through_mix and not delta   # SPEC: a delta vertex is never paired
        wo_l = bsdf.frame.world_to_local(wo)
        if bsdf.closure[0] == "diffuse":
            f, wi_l, p_b = R.diffuse_sample(bsdf.closure[1], su, wo_l, count)
        elif bsdf.closure[0] == "glossy":
            f, wi_l, p_b = R.glossy_sample(bsdf.closure[1], bsdf.closure[2], su, wo_l, count)
        elif bsdf.closure[0] == "mirror":                      # SPEC
            f, wi_l, p_b = mirror_sample(bsdf.closure[1], wo_l, count)
        else:                                                  # SPEC
            if roles is not None:
                roles.append(("glass_uy", su[1]))
            f, wi_l, p_b = glass_sample(bsdf.closure[1], bsdf.closure[2], su, wo_l, count)
        wi = bsdf.frame.local_to_world(wi_l)
        pdf = F(p_b * bsdf.choice_pdf)
        if pdf == 0:
            tick("scatter.pdf_zero")
            break
        tick("scatter.event")
        cosg = fabs(dot(ng, wi))
        ev_tmin = F(EPS / cosg)
        ev_beta = divs(scale(cosg, f), pdf)
        carry = None
        if pair and p_b > 0:
            carry = (divs(mul(beta, scale(fabs(dot(ns, wi)), f)), p_b), p_b)
        sel_u = sampler.next2d()
        take_env, sel_pdf, lid = False, ONE, None
        if env is not None:
            lu = sampler.next2d()
            sp = env.select_prob
            if not sc.lights or sel_u[0] < sp:
                take_env, sel_pdf = True, (sp if sc.lights else ONE)
            else:
                lid, lpdf = sc.select_light((F(F(sel_u[0] - sp) / F(ONE - sp)), sel_u[1]))
                lpdf = F(lpdf * F(ONE - sp))
        else:
            lid, lpdf = sc.select_light(sel_u)
            if lid is not None:
                lu = sampler.next2d()
        if take_env:
            ewi, Le, epdf, _ = env.sample(lu)
            if epdf <= 0:
                tick("env.pdf_nonpositive")
            else:
                fl = scale(fabs(dot(ns, ewi)), mul(Le, bsdf_evaluate(bsdf, wo, ewi, count)))
                p_l = F(sel_pdf * epdf)
                color = divs(mul(beta, fl), p_l)
                if R.is_black(color):
                    tick("spec.direct_black" if delta else "env.black")
                else:
                    if pair:
                        color = scale(M.power_weight(p_l, closure_pdf(bsdf.closure, wo_l, bsdf.frame.world_to_local(ewi))), color)
                    tr.shadow += 1
                    if tr.occlude(p, ewi, F(EPS / fabs(dot(ng, ewi))), INF):
                        tick("env.occluded")
                    else:
                        tick("env.lit")
                        L = add(L, color)
        elif lid is not None:
            ltri = sc.tris[lid]
            ls = R.light_sample(ltri, ltri.material[1], lu, p)
            if ls["pdf"] <= 0:
                tick("direct.pdf_nonpositive")
            else:
                lpdf = F(lpdf * ls["pdf"])
                fl = scale(fabs(dot(ns, ls["wi"])), mul(ls["L"], bsdf_evaluate(bsdf, wo, ls["wi"], count)))
                color = divs(mul(beta, fl), lpdf)
                if R.is_black(color):
                    tick("spec.direct_black" if delta else "direct.black")
                else:
                    if pair:
                        color = scale(M.power_weight(lpdf, closure_pdf(bsdf.closure, wo_l, bsdf.frame.world_to_local(ls["wi"]))), color)
                    tr.shadow += 1
                    if tr.occlude(ls["o"], ls["d"], ls["tmin"], ls["tmax"]):
                        tick("direct.occluded")
                    else:
                        tick("direct.lit")
                        L = add(L, color)
        else:
            tick("direct.no_light")
        if last and delta:                                     # SPEC: this vertex's ray is traced and counted
            tick("spec.ray_at_max_depth")
        beta = mul(beta, ev_beta)
        depth += 1
        via_delta = delta                                      # SPEC
        o, d, tmin, tmax = p, wi, ev_tmin, INF
    return add(L, Eterm)


def render_pixel(sc, env, x, y, spp, max_depth, ray_clamp=0.0, count=None, width=None, roles=None, mis=False,
                 samples=None):
    """mis_restate.render_pixel over this file's path_sample."""
    w = sc.camera.res[0] if width is None else width
    sampler = R.LCG((x + y * w) & R.M32)
    rad = BLACK
    weight = ZERO
    tr = R.Tracer(sc)
    first = {}
    for s in range(spp):
        rec = first if s == 0 else None
        L = path_sample(sc, sampler, x, y, max_depth, count, tr, rec, roles, env, mis)
        if ray_clamp > 0:
            L = R.clamp_radiance(L, ray_clamp)
        if samples is not None:
            samples.append(L)
        weight = F(weight + ONE)
        rad = add(rad, L)
    return dict(radiance=rad, weight=weight, seed=sampler.seed, closest=tr.closest, shadow=tr.shadow,
                ambiguous=tr.ambiguous, first=first)

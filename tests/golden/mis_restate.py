"""Multiple importance sampling of lights restated in numpy f32 on top of
ref_restate.py and env_restate.py.

The reference combines nothing: all light beyond the camera ray arrives through one next-event sample per
vertex, and a BSDF-sampled ray that reaches a lamp or leaves the scene adds nothing.  With `mis` on, direct
lighting at a paired vertex is the power-heuristic combination of the next-event sample and the BSDF sample
that the extension ray already is: no draw is added or moved, no ray is added or removed, so the final
sampler state and both ray counts of every pixel are the mis-off render's.  `path_sample` is
env_restate.path_sample statement for statement (ref_restate.path_sample when env is None) with the additions
marked `# MIS`.  All arithmetic is f32, unfused, in the written order.  It shares no code with the HIP library.

What the two images do not share in expectation.  At a Glossy vertex whose BSDF sample fails (pdf == 0) the
reference ends the path before direct lighting, so today's image lacks (1 - P_ok) * integral(Le f cos) there,
P_ok being the probability that the sample succeeds.  With MIS only the next-event share of that is missing,
since the BSDF-sampled share never passed through direct lighting.  So the two images differ in expectation
by (1 - P_ok) * integral(w_b Le f cos) >= 0 at Glossy vertices, the MIS image being the nearer to the
integral.  The reference's control flow is kept: direct lighting after a failed sample would move draws.
"""
import numpy as np

import env_restate as E
import ref_restate as R
from ref_restate import EPS, F, INF, INV_PI, add, divs, dot, fabs, mul, neg, normalize, scale, sub

ONE, FOUR = F(1.0), F(4.0)


def power_weight(a, b):
    """w(a, b) = 1 / (1 + (b / a) (b / a)), a the pdf of the strategy that drew the direction (a > 0):
    0 for b = inf, and never 0 / 0."""
    r = F(F(b) / F(a))
    return F(ONE / F(ONE + F(r * r)))


def closure_pdf(closure, wo, wi):
    """evaluate_pdf of the reference's closures (material.h, DiffuseBSDF and MicrofacetReflection), which its
    path tracer never calls; wo, wi in the shading frame, no choice_pdf."""
    if not R.same_hemisphere(wo, wi):
        return F(0.0)
    if closure[0] == "diffuse":
        return F(fabs(wi[1]) * INV_PI)
    wh = add(wo, wi)
    if wh[0] == 0 and wh[1] == 0 and wh[2] == 0:
        return F(0.0)
    wh = normalize(wh)
    if wh[1] < 0:
        wh = neg(wh)
    return F(F(R.ggx_d(closure[2], wh) * fabs(wh[1])) / F(FOUR * fabs(dot(wo, wh))))


def tri_select_pdf(sc):
    """Per triangle: the selection pdf of the light list's entries that name it (their sum, in list order, if it
    is listed more than once); 0 for a triangle no entry names."""
    out = {}
    n = len(sc.lights)
    for i, gid in enumerate(sc.lights):
        pdf = F(sc.dist.func[i] / F(sc.dist.func_int * F(n)))
        out[gid] = F(out[gid] + pdf) if gid in out else pdf
    return out


def path_sample(sc, sampler, px, py, max_depth, count=None, tracer=None, record=None, roles=None, env=None, mis=True):
    def tick(k):
        if count is not None:
            count[k] += 1
    tr = tracer if tracer is not None else R.Tracer(sc)
    if not hasattr(sc, "_mis_tri_sel"):
        sc._mis_tri_sel = tri_select_pdf(sc)
    L = (F(0.0),) * 3
    Eterm = (F(0.0),) * 3              # MIS: the terminal term of the carried pair
    carry = None                       # MIS: (T, p_b) of the extension ray
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
            if depth == 0 and env is not None:
                tick("miss.sky")
                Le, _, _ = env.eval(d)
                L = add(L, mul(beta, Le))
            else:
                tick("miss")
                if carry is not None and env is not None:      # MIS: the BSDF sample reached the environment
                    T, p_b = carry
                    Le, p_w, _ = env.eval(d)
                    p_l = F((env.select_prob if sc.lights else ONE) * p_w)
                    if p_l > 0:
                        tick("mis.term_env")
                        Eterm = scale(power_weight(p_b, p_l), mul(T, Le))
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
            if depth == 0:
                front = dot(neg(wo), ng) < 0
                if mat[2] or front:
                    tick("scatter.emit")
                    L = add(L, mul(beta, R.texture_evaluate(mat[1], tc)))
            elif carry is not None:                            # MIS: the BSDF sample reached an area light
                T, p_b = carry
                c = F(-dot(d, ng))
                po = sub(p, o)
                d2 = dot(po, po)
                sel = sc._mis_tri_sel.get(gid, F(0.0))
                if env is not None:
                    sel = F(sel * F(ONE - env.select_prob))
                p_l = F(sel * F(F(d2 / c) / tri.area()))
                if not c > 0:          # next-event estimation lights front faces only, whatever double_sided says
                    tick("mis.term_area_back")
                elif not p_l > 0:      # not in the light list, or a selection pdf of 0 or NaN
                    tick("mis.term_area_pdf_nonpositive")
                else:
                    tick("mis.term_area")
                    Eterm = scale(power_weight(p_b, p_l), mul(T, R.texture_evaluate(mat[1], tc)))
            break
        if not depth < max_depth:
            tick("scatter.max_depth")
            break
        through_mix = mat[0] == "mix"
        bsdf = R.get_bsdf(mat, cu1[0], tc, ng, ns, count)
        su = sampler.next2d()
        if bsdf is None:
            tick("scatter.mix_to_emissive")
            break
        # MIS: the vertex is paired unless it is the last one or was reached through a Mix (whose BSDF draw is
        # the selection draw, so its sample is not distributed by its stated pdf)
        pair = mis and depth + 1 < max_depth and not through_mix
        if mis and not depth + 1 < max_depth:
            tick("mis.unpaired_last")
        elif mis and through_mix:
            tick("mis.unpaired_mix")
        wo_l = bsdf.frame.world_to_local(wo)
        if bsdf.closure[0] == "diffuse":
            f, wi_l, p_b = R.diffuse_sample(bsdf.closure[1], su, wo_l, count)
        else:
            f, wi_l, p_b = R.glossy_sample(bsdf.closure[1], bsdf.closure[2], su, wo_l, count)
        wi = bsdf.frame.local_to_world(wi_l)
        pdf = F(p_b * bsdf.choice_pdf)                         # BSDF.sample's return; p_b is the value before it
        if pdf == 0:
            tick("scatter.pdf_zero")
            if pair:                                           # MIS: nothing is carried, and the path ends
                tick("mis.pb_nonpositive")
            break
        tick("scatter.event")
        cosg = fabs(dot(ng, wi))
        ev_tmin = F(EPS / cosg)
        ev_beta = divs(scale(cosg, f), pdf)
        carry = None
        if pair:
            if p_b > 0:
                carry = (divs(mul(beta, scale(fabs(dot(ns, wi)), f)), p_b), p_b)
            else:
                tick("mis.pb_nonpositive")
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
                fl = scale(fabs(dot(ns, ewi)), mul(Le, bsdf.evaluate(wo, ewi, count)))
                p_l = F(sel_pdf * epdf)
                color = divs(mul(beta, fl), p_l)
                if R.is_black(color):
                    tick("env.black")
                else:
                    if pair:                                   # MIS
                        color = scale(power_weight(p_l, closure_pdf(bsdf.closure, wo_l, bsdf.frame.world_to_local(ewi))), color)
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
                fl = scale(fabs(dot(ns, ls["wi"])), mul(ls["L"], bsdf.evaluate(wo, ls["wi"], count)))
                color = divs(mul(beta, fl), lpdf)
                if R.is_black(color):
                    tick("direct.black")
                else:
                    if pair:                                   # MIS
                        color = scale(power_weight(lpdf, closure_pdf(bsdf.closure, wo_l, bsdf.frame.world_to_local(ls["wi"]))), color)
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
    return add(L, Eterm)               # the terminal event ends the path: its term is the last in path order


def render_pixel(sc, env, x, y, spp, max_depth, ray_clamp=0.0, count=None, width=None, roles=None, mis=True,
                 samples=None):
    """env_restate.render_pixel with the switch; `samples`, a list, collects every sample's clamped L."""
    w = sc.camera.res[0] if width is None else width
    sampler = R.LCG((x + y * w) & R.M32)
    rad = (F(0.0),) * 3
    weight = F(0.0)
    tr = R.Tracer(sc)
    first = {}
    for s in range(spp):
        rec = first if s == 0 else None
        L = path_sample(sc, sampler, x, y, max_depth, count, tr, rec, roles, env, mis)
        if ray_clamp > 0:
            L = R.clamp_radiance(L, ray_clamp)
        if samples is not None:
            samples.append(L)
        weight = F(weight + F(1.0))
        rad = add(rad, L)
    return dict(radiance=rad, weight=weight, seed=sampler.seed, closest=tr.closest, shadow=tr.shadow,
                ambiguous=tr.ambiguous, first=first)

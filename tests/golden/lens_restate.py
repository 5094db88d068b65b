"""The reference's thin lens (kernel/camera.h:43-44, 67-86) beside ref_restate.py, which states the camera
with lens_radius 0, and the AO integrator's pixel loop, which ref_restate.py has none of.

LensCamera is ref_restate.Camera with the two fields the reference's kernel camera holds and its camera node
never sets.  The path loops of ref_restate, env_restate, mis_restate and specular_restate all call
sc.camera.generate_ray(u1, u2, raster), so a restated scene whose camera is a LensCamera runs through all
four unchanged (with_lens below swaps it in).  Same conventions as ref_restate.py: one f32 operation per
reference operation, unfused, arguments left to right.
"""
import numpy as np

import ref_restate as R

F = np.float32


class LensCamera(R.Camera):
    """PerspectiveCamera with lens_radius and focal_distance (camera.h:43-44)."""

    def __init__(self, position, rotation_deg, fov_deg, resolution, lens_radius=0.0, focal_distance=0.0):
        super().__init__(position, rotation_deg, fov_deg, resolution)
        self.lens_radius = F(lens_radius)
        self.focal_distance = F(focal_distance)

    @property
    def active(self):
        """camera.h:75."""
        return bool(self.lens_radius > 0 and self.focal_distance > 0)

    def camera_space_ray(self, u1, u2, raster):
        """camera.h:69-80: the ray before c2w -> (o, d)."""
        pf = (F(F(raster[0]) + u2[0]), F(F(raster[1]) + u2[1]))
        p = R.apply_point(self.r2c, (pf[0], pf[1], F(0.0)))
        o = (F(0.0), F(0.0), F(0.0))
        d = R.normalize(R.sub((p[0], p[1], F(0.0)), (F(0.0), F(0.0), F(1.0))))
        if self.active:
            pl = R.scale(self.lens_radius, R.concentric_disk(u1))     # :69, Array * scalar
            ft = F(self.focal_distance / R.fabs(d[2]))                # :76
            p_focus = R.add(o, R.scale(ft, d))                        # :77, Ray::operator(): o + t * d
            o = (pl[0], pl[1], F(0.0))                                # :78
            d = R.normalize(R.sub(p_focus, o))                        # :79
        return o, d

    def generate_ray(self, u1, u2, raster):
        """camera.h:67-86 -> (o, d) in world space; tmin and tmax stay the path loop's Eps and Inf."""
        o, d = self.camera_space_ray(u1, u2, raster)
        return R.apply_point(self.c2w, o), R.apply_vector(self.c2w, d)


def lens_camera_of(cam):
    """A scene description's PerspectiveCamera (akari_amd.scene) restated."""
    return LensCamera(cam.position, cam.rotation, cam.fov, cam.resolution, getattr(cam, "lens_radius", 0.0),
                      getattr(cam, "focal_distance", 0.0))


def with_lens(restated_scene, cam):
    """The restated scene (RefScene, SpecScene, ...) with its camera replaced by `cam`'s LensCamera."""
    restated_scene.camera = lens_camera_of(cam)
    return restated_scene


# ----------------------------------------------------------------------------- AO integrator
def ao_sample(sc, camera, sampler, px, py, occlude, tracer):
    """cpu::AmbientOcclusion::render's Li over one camera sample (kernel/integrators/cpu/integrator.cpp:43-60,
    77-79).  The two next2d() of :78 are taken left to right, lens draw first, as pathtracer.h:61-64 spells
    out and oracle/akr_oracle.cpp reads it.  -> 0.0 or 1.0 (every channel of the Spectrum)."""
    u1 = sampler.next2d()
    u2 = sampler.next2d()
    o, d = camera.generate_ray(u1, u2, (px, py))
    tracer.closest += 1
    hit = tracer.intersect(o, d, R.EPS, R.INF)                       # :46
    if hit is None:
        return F(0.0)                                                # :58
    gid, _, hu, hv = hit
    tri = sc.tris[gid]
    frame = R.Frame(tri.ng())                                        # :48
    w = R.cosine_hemisphere(sampler.next2d())                        # :49
    w = frame.local_to_world(w)                                      # :50
    tracer.shadow += 1
    h2 = tracer.intersect(tri.p((hu, hv)), w, R.EPS, R.INF)          # :51-53, Ray3f(o, d): tmin Eps, tmax Inf
    if h2 is not None and h2[1] < F(occlude):
        return F(0.0)
    return F(1.0)


def ao_pixel(sc, camera, x, y, spp, occlude=np.inf, width=None):
    """integrator.cpp:72-81 for one pixel: the sampler starts at x + y * width and runs through the samples;
    the tile adds each L with weight 1.  -> dict(radiance (3), weight, seed, closest, shadow, ambiguous)."""
    w = camera.res[0] if width is None else width
    sampler = R.LCG((x + y * w) & R.M32)
    tr = R.Tracer(sc)
    acc, weight = F(0.0), F(0.0)
    for _ in range(spp):
        acc = F(acc + ao_sample(sc, camera, sampler, x, y, occlude, tr))
        weight = F(weight + F(1.0))
    return dict(radiance=(acc, acc, acc), weight=weight, seed=sampler.seed, closest=tr.closest, shadow=tr.shadow,
                ambiguous=tr.ambiguous)

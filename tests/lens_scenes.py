"""Scenes seen through a thin lens: what tests/golden/make_lens_golden.py restates and
the device tests upload."""
import helpers
from akari_amd import scene

RES = (24, 24)


def lens_box(resolution=RES):
    """The Cornell fixture from a moved and turned camera, so that apply_point's translation and all three
    rotations of c2w matter, focused on the blocks (fov 15, lens radius 0.3, focal distance 8)."""
    sc = helpers.cornell(resolution)
    sc.camera = scene.PerspectiveCamera(position=(0.3, 1.2, 9.0), rotation=(3.0, -2.0, 5.0), fov=15.0,
                                        resolution=tuple(resolution), lens_radius=0.3, focal_distance=8.0)
    return sc


def _near_box(resolution):
    """The Cornell fixture from just outside its open side: fov 80, a plane of focus half a unit away."""
    sc = helpers.cornell(resolution)
    sc.camera = scene.PerspectiveCamera(position=(0.1, 1.0, 2.6), rotation=(0.0, 0.0, 0.0), fov=80.0,
                                        resolution=tuple(resolution), lens_radius=0.2, focal_distance=0.5)
    return sc


def lens_wide(resolution=(24, 16)):
    """r2c's branch for a frame wider than high."""
    return _near_box(resolution)


def lens_tall(resolution=(16, 24)):
    """... and for one higher than wide."""
    return _near_box(resolution)


def lens_sky_spec(resolution=RES, area=True):
    """specular_scenes.sky_spec (Mirror and Glass under the open sky, two small lamps) with its camera given a
    lens focused on the box; the caller adds the EnvironmentLight as make_specular_golden.build_scene does.
    The radius is a unit: a sky pixel changes only when a sample crosses a texel of the 8 x 8 map, and at 0.15
    only 27 % of the frame differed from the pinhole's (0.5: 53 %, 1.0: 77 %)."""
    import specular_scenes
    sc = specular_scenes.sky_spec(resolution, area=area)
    sc.camera.lens_radius = 1.0
    sc.camera.focal_distance = 4.0
    return sc


def lens_ao(resolution=RES):
    """The Cornell fixture under the AO integrator, from lens_wide's camera.  An AO film holds
    0 .. spp per pixel, so few pixels can differ from the pinhole's where the box is in focus (lens_box's camera:
    12 %, and 28 % at radius 0.6 with occlude 0.6); this camera focuses far in front of the box, and the finite
    occlude distance takes the closest-hit AO branch and leaves both answers common."""
    sc = _near_box(resolution)
    sc.integrator = scene.AOIntegrator(spp=4, occlude=0.6)
    return sc


def pinhole(sc):
    """The same scene without its lens."""
    sc.camera.lens_radius = 0.0
    sc.camera.focal_distance = 0.0
    return sc

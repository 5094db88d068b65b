"""Scenes with Mirror and Glass materials: what tests/golden/make_specular_golden.py
restates and the device tests upload."""
import numpy as np

import helpers
from akari_amd import scene

RES = (24, 24)
CT = scene.ConstantTexture


def fraction_image(seed, h=6, w=5):
    """An h x w image of Mix fractions in [0.25, 0.75) in steps of 1 / 256 (exact in f32), from an integer hash."""
    k = (np.arange(h * w, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B1)) * np.uint64(2654435761)
    k = (k & np.uint64(0xFFFFFFFF)) >> np.uint64(9)
    f = ((k & np.uint64(0x7F)).astype(np.float32) + np.float32(64)) / np.float32(256)
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = f.reshape(h, w, 1)
    return scene.ImageTexture(img)


def mirror_box(resolution=RES):
    """The Cornell fixture with the tall block a Mirror: the lamp is seen in it."""
    sc = helpers.cornell(resolution)
    sc.shapes[0].materials[6] = scene.MirrorMaterial(CT([0.9, 0.85, 0.8]))
    return sc


def glass_box(resolution=RES):
    """The Cornell fixture with the short block a Glass of ior 1.5."""
    sc = helpers.cornell(resolution)
    sc.shapes[0].materials[5] = scene.GlassMaterial(CT([0.95, 0.97, 1.0]), 1.5)
    return sc


def mirror_glass_box(resolution=RES):
    """Both: the 1080p measurement's scene."""
    sc = mirror_box(resolution)
    sc.shapes[0].materials[5] = scene.GlassMaterial(CT([0.95, 0.97, 1.0]), 1.5)
    return sc


def mixed_spec(resolution=RES):
    """Mix(Diffuse, Mirror) on the tall block and Mix(Glossy, Glass) on the short one, both with image
    fractions, and a double-sided lamp."""
    sc = helpers.cornell(resolution)
    m = sc.shapes[0].materials
    m[6] = scene.MixMaterial(fraction_image(1), scene.DiffuseMaterial(CT([0.2, 0.7, 0.2])),
                             scene.MirrorMaterial(CT([0.9, 0.9, 0.9])))
    m[5] = scene.MixMaterial(fraction_image(2), scene.GlossyMaterial(CT([0.9, 0.8, 0.7]), CT([0.4, 0.4, 0.4])),
                             scene.GlassMaterial(CT([1.0, 1.0, 1.0]), 1.33))
    m[7] = scene.EmissiveMaterial(CT([17.0, 12.0, 4.0]), double_sided=True)
    return sc


def sky_spec(resolution=RES, area=False):
    """make_env_golden's ground quad and box in the open, the box's side faces Mirror and its top and far side
    Glass.  area: two small lamps between the camera and the box that face the camera, one one-sided and one
    double-sided; rays the box's near face reflects meet them from behind."""
    import make_env_golden as ME
    sc = ME.sky_scene(resolution)
    mesh = sc.shapes[0]
    mesh.materials[1] = scene.MirrorMaterial(CT([0.9, 0.9, 0.9]))
    mesh.materials[2] = scene.GlassMaterial(CT([0.9, 1.0, 0.95]), 1.5)
    if area:
        x, y0, y1 = -0.5, 0.55, 0.85
        tris = [[(x, y0, -1.0), (x, y0, -0.3), (x, y1, -1.0)], [(x, y0, -0.2), (x, y0, 0.5), (x, y1, -0.2)]]
        mesh.materials += [scene.EmissiveMaterial(CT([6.0, 2.0, 2.0]), double_sided=False),
                           scene.EmissiveMaterial(CT([2.0, 6.0, 2.0]), double_sided=True)]
        nv = len(mesh.vertices)
        mesh.vertices = np.concatenate([mesh.vertices, np.array(tris, np.float32).reshape(-1, 3)])
        mesh.indices = np.concatenate([mesh.indices, np.arange(nv, nv + 6, dtype=np.int32).reshape(2, 3)])
        mesh.normals = np.concatenate([mesh.normals, np.tile(np.array([-1, 0, 0] * 3, np.float32), (2, 1))])
        mesh.texcoords = np.concatenate([mesh.texcoords, np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (2, 1))])
        mesh.material_indices = np.concatenate([mesh.material_indices, np.array([3, 4], np.int32)])
    return sc


def facing_mirror(resolution=(8, 8)):
    """A mirror square at z = 0 seen head-on from z = 4, and a large one-sided lamp at z = 6 behind the camera
    that faces the mirror: every pixel on the mirror reflects into the lamp."""
    mats = [scene.MirrorMaterial(CT([0.8, 0.6, 0.4])), scene.EmissiveMaterial(CT([3.0, 2.0, 1.0]))]
    tris = [[(-1, -1, 0), (1, -1, 0), (1, 1, 0)], [(-1, -1, 0), (1, 1, 0), (-1, 1, 0)],
            [(-40, -40, 6), (-40, 40, 6), (40, 40, 6)], [(-40, -40, 6), (40, 40, 6), (40, -40, 6)]]
    cam = scene.PerspectiveCamera(position=(0.013, 0.007, 4.0), rotation=(0.0, 0.0, 0.0), fov=20.0,
                                  resolution=tuple(resolution))
    return helpers.tri_scene(tris, mats, [0, 0, 1, 1], cam)


def glass_slab(ior=1.5, resolution=(4, 4)):
    """A slab of Glass (two parallel squares, z = 0 and z = -0.5) between the camera at z = 4 and a large
    one-sided lamp at z = -3 that faces it; 1 degree of view, so every ray is within half a degree of normal."""
    mats = [scene.GlassMaterial(CT([1.0, 1.0, 1.0]), ior), scene.EmissiveMaterial(CT([2.0, 2.0, 2.0]))]
    tris = [[(-1, -1, 0), (1, -1, 0), (1, 1, 0)], [(-1, -1, 0), (1, 1, 0), (-1, 1, 0)],
            [(-1, -1, -0.5), (1, 1, -0.5), (1, -1, -0.5)], [(-1, -1, -0.5), (-1, 1, -0.5), (1, 1, -0.5)],
            [(-40, -40, -3), (40, -40, -3), (40, 40, -3)], [(-40, -40, -3), (40, 40, -3), (-40, 40, -3)]]
    cam = scene.PerspectiveCamera(position=(0.013, 0.007, 4.0), rotation=(0.0, 0.0, 0.0), fov=1.0,
                                  resolution=tuple(resolution))
    return helpers.tri_scene(tris, mats, [0, 0, 0, 0, 1, 1], cam)

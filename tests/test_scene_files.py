"""The reference's own scene files (BASELINE.json configs[0]):
resources/data/cornell_box/scene.akari (importing cornell_box.akari, naming
CornellBox-Original.obj.mesh) and resources/example.akari (importing foo.akari), parsed with the
restated .akari language (core/parser.cpp:150-363), resolve to the committed golden
(tests/golden/reference_scenes.json, made by make_scene_golden.py from the files themselves, which
stay in the reference tree).  Here the golden is met from two sides: the renderer's built-in
cornell_scene() restates it, and scene files written for this project in the same language (two
modules each, below) parse to it value for value and compile to the same arrays."""
import json
import sys

import numpy as np

from akari_amd import scene
from conftest import CORNELL_MESH, GOLDEN

sys.path.insert(0, str(GOLDEN))
from scene_summary import summarize  # noqa: E402
import make_scene_golden  # noqa: E402

# The Cornell box of the golden as this project writes it: the mesh module keeps the shared white in a
# local, comments between the entries and a comma after the last one; the scene module reaches the
# mesh through the import's name.
CORNELL_MESH_MODULE = """
// Cornell box: the eight material slots of the mesh, in slot order
let white = [0.725, 0.71, 0.68]   // floor, ceiling, back wall and both boxes
export lamp = EmissiveMaterial { color: [17, 12, 4] }
export mesh = AkariMesh {
  materials: [
    DiffuseMaterial { color: [0.63, 0.065, 0.05] },    // 0 left wall
    DiffuseMaterial { color: [0.14, 0.45, 0.091] },    // 1 right wall
    // 2-6: floor, ceiling, back wall, short box, tall box
    DiffuseMaterial { color: $white }, DiffuseMaterial { color: $white }, DiffuseMaterial { color: $white },
    DiffuseMaterial { color: $white }, DiffuseMaterial { color: $white },
    $lamp,   // 7
  ],
  path: "MESH"
}
"""
CORNELL_SCENE_MODULE = """
import "box.akari" as cbox
// 1024 x 1024, 16 spp in one tile
export view = PerspectiveCamera { resolution: [1024, 1024], fov: 15, rotation: [0, 0, 0], position: [0, 1, 9] }
export scene = Scene {
    shapes: [ $cbox.mesh ],
    output: "out.png",
    integrator: Path { tile_size: 1024, max_depth: 5, spp: 16 },
    camera: $view
}
"""
# import ... as, a $module.var reference inside an array, and an object node of a type the renderer
# does not know (kept as a generic node)
VALUES_MODULE = "// one exported number\nexport n = 444\n"
VALUES_MAIN = """
import "values.akari" as v
export obj = Camera { position: [1, 2, 3] }
export bar = [ $v.n, 123 ]
"""


def _golden():
    return json.loads((GOLDEN / "reference_scenes.json").read_text())


def test_golden_cornell_equals_builtin_cornell_scene():
    """The golden resolution of scene.akari is exactly cornell_scene() at the file's settings
    (1024^2, spp 16, max_depth 5, tile 1024) over the committed .mesh fixture."""
    g = _golden()["cornell_scene"]
    mine = summarize(scene.cornell_scene(CORNELL_MESH, resolution=(1024, 1024), spp=16, max_depth=5))
    mine = json.loads(json.dumps(mine))
    assert mine == g


def test_golden_cornell_compiles_to_the_reference_light_list():
    """SceneNode::compile (core/nodes/scene.cpp:51-92): the two emissive triangles of the light
    (material slot 7) become the area lights, with power 2 * area * uv-area * luminance(Le)."""
    cs = scene.compile_scene(scene.cornell_scene(CORNELL_MESH, resolution=(1024, 1024)))
    mi = np.asarray(_golden()["cornell_scene"]["shapes"][0]["material_indices"])
    assert sorted(np.asarray(cs.light_gid).tolist()) == np.flatnonzero(mi == 7).tolist()
    assert len(cs.power) == 2 and np.all(np.asarray(cs.power) > 0)


def test_scene_file_parses_to_the_golden_and_compiles_like_the_builtin(tmp_path):
    (tmp_path / "box.akari").write_text(CORNELL_MESH_MODULE.replace("MESH", str(CORNELL_MESH)))
    (tmp_path / "scene.akari").write_text(CORNELL_SCENE_MODULE)
    sc = scene.load_scene_file(tmp_path / "scene.akari")
    assert json.loads(json.dumps(summarize(sc))) == _golden()["cornell_scene"]
    # and renders the same scene as the built-in restatement: identical compiled arrays
    a = scene.compile_scene(sc)
    b = scene.compile_scene(scene.cornell_scene(CORNELL_MESH, resolution=(1024, 1024)))
    for f in ("vertices", "indices", "normals", "texcoords", "matid", "light_gid", "power"):
        assert np.array_equal(np.asarray(getattr(a, f)), np.asarray(getattr(b, f))), f
    assert a.camera == b.camera


def test_module_file_parses_to_the_golden(tmp_path):
    """import ... as, $module.var references and a generic object node."""
    (tmp_path / "values.akari").write_text(VALUES_MODULE)
    (tmp_path / "main.akari").write_text(VALUES_MAIN)
    got = json.loads(json.dumps(make_scene_golden.example_summary(tmp_path / "main.akari")))
    assert got == _golden()["example"]
    assert got["bar"] == [444.0, 123.0] and got["obj"]["fields"]["position"] == [1.0, 2.0, 3.0]

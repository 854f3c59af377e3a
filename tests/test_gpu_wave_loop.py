"""The traversal loop of the persistent kernels at its edges (csrc/rt_device.h: trav_step_wave, trav_classes; the loops of k_megakernel,
k_wf_finish and path_rounds). The exit test and the vote are arithmetic on lane masks, and the first step of an iteration takes its leaf
class from the exit test's mask: a lane that is neither at an inner node nor done. That holds only while the masks speak of the same lanes,
so the shapes here are the ones where the classes are lopsided:
  a tile smaller than a wave         most lanes of the only wave never hold a ray: they are done, and must be in no class;
  depth 1                            every shading round ends every path: each traversal phase starts with all live lanes at the root;
  depth 10 on two-triangle walls     a leaf is a whole wall directly under a node of walls: leaf lanes outnumber inner lanes in the vote;
  forced slices on a 16 x 16 tile    lanes that wait for their pixel's state stand beside lanes that trace, and raise the threshold.
Both one-launch renderers render each shape, and the path query traces the rays of the same camera: frames, images, radiances, states and
ray counts are the CPU oracle's, bit for bit."""
import numpy as np
import pytest

from rtamd import abi
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer
from test_path_query import get_ray_model, pixel_seed_model

pytestmark = pytest.mark.gpu
f32 = np.float32
KINDS = ((WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT), (MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL))

SHAPES = {  # name -> (scene, keywords, width, height, spp, depth, the oracle walks its BVH, forced slices)
    "below_a_wave": ("cornell", {}, 5, 3, 2, 5, False, (-1,)),
    "depth_1": ("cornell", {}, 64, 8, 3, 1, False, (-1,)),
    "walls_depth_10": ("atrium_tilted", {"detail": 1}, 64, 8, 3, 10, True, (-1,)),
    "forced_slices": ("cornell", {}, 16, 16, 8, 5, False, (2, 8)),
}

_SHARED = {}


def shape(name, oracle, scene_cache):
    """(description, device scene, camera, the oracle's frames per renderer kind, camera rays, the oracle's path query on them), once per module"""
    if name not in _SHARED:
        sname, kw, w, h, spp, depth, use_bvh, _ = SHAPES[name]
        sd = scene_cache(sname, **kw)
        osc = oracle.OracleScene(sd)
        ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
        frames = {kind: osc.render(ocam, kind, depth, spp, use_bvh=use_bvh) for _, kind in KINDS}
        cam = Camera.for_scene(sd, (w, h))
        ys, xs = np.mgrid[0:h, 0:w]
        state = pixel_seed_model(xs.ravel(), ys.ravel(), w, h, megakernel=True)
        d, _ = get_ray_model(cam.c, xs.ravel(), ys.ravel(), state)
        org = np.tile(np.array(list(cam.c.center), f32), (w * h, 1))
        rays = (org, d, state)
        paths = osc.trace_paths(org, d, state, depth, samples=spp)
        _SHARED[name] = (sd, Scene(sd, device=0), cam, frames, rays, paths)
    return _SHARED[name]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    yield
    for entry in _SHARED.values():
        entry[1].close()
    _SHARED.clear()


@pytest.mark.parametrize("cls,kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_frame_is_the_oracles(oracle, scene_cache, name, cls, kind):
    _, _, w, h, spp, depth, _, slicings = SHAPES[name]
    _, scene, cam, frames, _, _ = shape(name, oracle, scene_cache)
    f, b, rays = frames[kind]
    assert rays > w * h * spp or depth == 1  # paths do bounce
    r = cls(scene, (w, h), depth, spp)
    try:
        for slices in slicings:
            if slices >= 0:
                r.set_schedule(pixel_slices=slices)
            fr = r.render_frame(cam)
            what = f"{name} {cls.__name__}, slices {slices}"
            if slices >= 2:
                assert fr.pixel_slices == slices, what
            assert fr.rays == rays, f"{what}: {fr.rays} rays, the oracle {rays}"
            np.testing.assert_array_equal(fr.rgba_f32, f, err_msg=what)
            np.testing.assert_array_equal(fr.rgba_u8, b, err_msg=what)
    finally:
        r.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_path_query_on_the_cameras_rays_is_the_oracles(oracle, scene_cache, name):
    _, _, w, h, spp, depth, _, _ = SHAPES[name]
    _, scene, _, _, (org, d, state), want = shape(name, oracle, scene_cache)
    got = scene.trace_paths(org, d, state, depth, samples=spp)
    assert int(want["rays"].astype(np.uint64).sum()) >= w * h * spp
    for k in ("radiance", "rng", "rays"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {k}")

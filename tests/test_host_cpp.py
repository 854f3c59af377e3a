"""CPU tests of the C++ host side: GLB loader + texture baker, PNG codec and the
`raytracer` CLI's argument handling. The GPU half (CLI end to end) is in test_gpu_cli.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.glb_export import export_glb

REPO = Path(__file__).resolve().parent.parent
HOST = REPO / "sycl-ray-tracer_amd" / "host" / "build"


@pytest.fixture(scope="module")
def hostlib(rtlib):
    p = HOST / "librt_host.so"
    if not p.exists():
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(str(p))
    lib.rth_last_error.restype = C.c_char_p
    lib.rth_load_glb.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.rth_scene_free.argtypes = [C.c_void_p]
    lib.rth_scene_desc.argtypes = [C.c_void_p, C.POINTER(abi.rt_scene_desc)]
    lib.rth_scene_camera.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.rth_write_png.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]
    lib.rth_decode_png.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_size_t]
    lib.rth_resize_to_layer.argtypes = [C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]
    return lib


class CppScene:
    """A scene loaded by the C++ loader, viewed as numpy arrays + usable as a SceneDesc for the oracle."""

    def __init__(self, lib, path):
        self.lib, self.h = lib, C.c_void_p()
        if lib.rth_load_glb(str(path).encode(), C.byref(self.h)) != 0:
            raise RuntimeError(lib.rth_last_error().decode())
        d = abi.rt_scene_desc()
        lib.rth_scene_desc(self.h, C.byref(d))
        self.c = d
        npf = lambda p, n: np.ctypeslib.as_array(p, (n,)).copy() if n else np.zeros(0, np.float32)
        self.positions = npf(d.positions, 3 * d.n_vertices).reshape(-1, 3)
        self.normals = npf(d.normals, 3 * d.n_vertices).reshape(-1, 3)
        self.uvs = npf(d.uvs, 2 * d.n_vertices).reshape(-1, 2)
        self.indices = np.ctypeslib.as_array(d.indices, (3 * d.n_triangles,)).copy().reshape(-1, 3)
        self.tri_instance = np.ctypeslib.as_array(d.tri_instance, (d.n_triangles,)).copy()
        self.instances = [d.instances[i] for i in range(d.n_instances)]
        self.materials = [d.materials[i] for i in range(d.n_materials)]
        pos, dr = (C.c_float * 3)(), (C.c_float * 3)()
        focal, has = C.c_float(), C.c_int()
        lib.rth_scene_camera(self.h, pos, dr, C.byref(focal), C.byref(has))
        self.camera = scenes.CameraPose(tuple(pos), tuple(dr), focal.value)
        self.has_camera = bool(has.value)

    def to_c(self):  # lets oracle.OracleScene consume the C++ loader's arrays directly
        return self.c

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.rth_scene_free(self.h)


@pytest.mark.parametrize("name", ["triangle", "cube"])
def test_cpp_loader_equals_python_loader_bitwise(hostlib, scene_cache, name):
    sd = scene_cache(name)
    cs = CppScene(hostlib, REPO / "assets" / f"{name}.glb")
    np.testing.assert_array_equal(cs.positions, sd.positions)
    np.testing.assert_array_equal(cs.normals, sd.normals)
    np.testing.assert_array_equal(cs.uvs, sd.uvs)
    np.testing.assert_array_equal(cs.indices, sd.indices)
    np.testing.assert_array_equal(cs.tri_instance, sd.tri_instance)
    py = sd.to_c()
    assert cs.c.n_instances == py.n_instances and cs.c.n_materials == py.n_materials and cs.c.n_layers == 0
    for i in range(py.n_instances):
        assert bytes(cs.instances[i]) == bytes(py.instances[i])
    for i in range(py.n_materials):
        assert bytes(cs.materials[i]) == bytes(py.materials[i])
    assert list(cs.c.sky) == list(py.sky)
    assert not cs.has_camera  # neither shipped asset has one: documented defaults apply
    np.testing.assert_allclose(cs.camera.position, sd.camera.position, rtol=0, atol=1e-7)
    np.testing.assert_array_equal(np.float32(cs.camera.direction), np.float32(sd.camera.direction))


@pytest.mark.parametrize("name,kw,w,h", [("cornell", {}, 40, 40), ("atrium", {"detail": 1}, 48, 27)])
def test_exported_glb_renders_identically_through_the_cpp_loader(hostlib, oracle, scene_cache, tmp_path, name, kw, w, h):
    """generator -> GLB (instancing, rotations, emissive/ior extensions, PNG textures, sky extras, camera node)
    -> C++ loader: the oracle renders the same image from both descriptions."""
    sd = scene_cache(name, **kw)
    path = tmp_path / f"{name}.glb"
    export_glb(sd, path)
    cs = CppScene(hostlib, path)
    assert cs.c.n_triangles == sd.n_triangles and cs.c.n_layers == sd.textures.shape[0]
    if sd.textures.shape[0]:
        tex = np.ctypeslib.as_array(cs.c.textures, (cs.c.n_layers, 512, 512, 4))
        np.testing.assert_array_equal(tex, sd.textures)  # 512x512 PNGs are baked without resampling
    assert cs.has_camera
    np.testing.assert_allclose(cs.camera.position, np.float32(sd.camera.position), atol=1e-6)
    dn = np.array(sd.camera.direction) / np.linalg.norm(sd.camera.direction)
    np.testing.assert_allclose(cs.camera.direction, dn, atol=1e-6)
    np.testing.assert_allclose(cs.camera.focal_length, sd.camera.focal_length, rtol=1e-6)
    cam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    a = oracle.OracleScene(sd).render(cam, 0, 6, 2)
    b = oracle.OracleScene(cs).render(cam, 0, 6, 2)
    assert a[2] == b[2]
    np.testing.assert_array_equal(a[0], b[0])


def test_loader_error_paths(hostlib, tmp_path):
    h = C.c_void_p()
    assert hostlib.rth_load_glb(str(tmp_path / "missing.glb").encode(), C.byref(h)) != 0
    assert b"cannot open" in hostlib.rth_last_error()
    bad = tmp_path / "bad.glb"
    bad.write_bytes(b"not a glb file at all.....")
    assert hostlib.rth_load_glb(str(bad).encode(), C.byref(h)) != 0
    assert b"GLB" in hostlib.rth_last_error()
    trunc = tmp_path / "trunc.glb"
    trunc.write_bytes((REPO / "assets" / "cube.glb").read_bytes()[:600])
    assert hostlib.rth_load_glb(str(trunc).encode(), C.byref(h)) != 0


def _craft_glb(path, js, bin_chunk=b""):
    from test_ref_gltf import glb_bytes  # the container writer lives with the crafted files of tests/test_ref_gltf.py
    path.write_bytes(glb_bytes(js, bin_chunk))


def test_loader_rejects_numbers_that_would_wrap_the_bounds_checks(hostlib, tmp_path):
    """count / byteOffset / byteStride / byteLength come from JSON doubles. Values whose products wrap
    around in size_t (count = 2^61 with stride 8), negative or non-finite values, and an image view whose offset + length
    wraps must all be refused with an error, never read out of bounds; a deeply nested document must not overflow the stack."""
    import struct
    tri = struct.pack("<9f", 0, 0, 0, 1, 0, 0, 0, 1, 0)
    nrm = struct.pack("<9f", 0, 0, 1, 0, 0, 1, 0, 0, 1)
    uv = struct.pack("<6f", 0, 0, 1, 0, 0, 1)
    idx = struct.pack("<3H", 0, 1, 2) + b"\0\0"
    blob = tri + nrm + uv + idx

    def doc(**over):
        views = [{"buffer": 0, "byteOffset": 0, "byteLength": 36}, {"buffer": 0, "byteOffset": 36, "byteLength": 36},
                 {"buffer": 0, "byteOffset": 72, "byteLength": 24}, {"buffer": 0, "byteOffset": 96, "byteLength": 6}]
        accs = [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"}, {"bufferView": 1, "componentType": 5126, "count": 3, "type": "VEC3"},
                {"bufferView": 2, "componentType": 5126, "count": 3, "type": "VEC2"}, {"bufferView": 3, "componentType": 5123, "count": 3, "type": "SCALAR"}]
        d = {"asset": {"version": "2.0"}, "buffers": [{"byteLength": len(blob)}], "bufferViews": views, "accessors": accs,
             "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2}, "indices": 3}]}],
             "nodes": [{"mesh": 0}], "scenes": [{"nodes": [0]}], "scene": 0}
        for k, v in over.items():
            a, i, f = k.split("__")
            d[a][int(i)][f] = v
        return d

    h = C.c_void_p()
    good = tmp_path / "good.glb"
    _craft_glb(good, doc(), blob)
    assert hostlib.rth_load_glb(str(good).encode(), C.byref(h)) == 0, hostlib.rth_last_error()
    hostlib.rth_scene_free(h)
    bad_cases = {
        "count_2p61_stride8": doc(accessors__0__count=2 ** 61, bufferViews__0__byteStride=8),  # (count-1)*stride wraps to a small number
        "count_huge": doc(accessors__3__count=1e300),
        "count_negative": doc(accessors__0__count=-3),
        "offset_negative": doc(bufferViews__1__byteOffset=-36),
        "offset_2p64": doc(accessors__2__byteOffset=2.0 ** 64),
        "stride_huge": doc(bufferViews__0__byteStride=2 ** 63),
        "index_of_node_negative": {**doc(), "scenes": [{"nodes": [-1]}]},
        "index_of_node_huge": {**doc(), "scenes": [{"nodes": [1e30]}]},
    }
    for name, d in bad_cases.items():
        pth = tmp_path / f"{name}.glb"
        _craft_glb(pth, d, blob)
        assert hostlib.rth_load_glb(str(pth).encode(), C.byref(h)) != 0, name
        assert hostlib.rth_last_error(), name
    # image buffer view whose offset + length wraps around
    d = doc()
    d["images"] = [{"bufferView": 4, "mimeType": "image/png"}]
    d["bufferViews"].append({"buffer": 0, "byteOffset": 8, "byteLength": 2.0 ** 64 - 4})
    _craft_glb(tmp_path / "img_wrap.glb", d, blob)
    assert hostlib.rth_load_glb(str(tmp_path / "img_wrap.glb").encode(), C.byref(h)) != 0
    # NaN is not valid JSON; strtod would accept it: must be an error, not a cast of NaN
    raw = b'{"asset":{"version":"2.0"},"accessors":[{"count":nan}],"scenes":[{"nodes":[]}]}'
    _craft_glb(tmp_path / "nan.glb", raw, blob)
    assert hostlib.rth_load_glb(str(tmp_path / "nan.glb").encode(), C.byref(h)) != 0
    # 100k nested arrays: a parse error (depth limit), not a stack overflow
    _craft_glb(tmp_path / "deep.glb", b"[" * 100000 + b"]" * 100000, b"")
    assert hostlib.rth_load_glb(str(tmp_path / "deep.glb").encode(), C.byref(h)) != 0
    assert b"nesting" in hostlib.rth_last_error()


def test_metallic_threshold_is_compared_in_double_like_the_reference(hostlib, tmp_path):
    """src/scene.cpp:219 compares the double metallicFactor with 0.01f promoted to double (0.00999999977648...): a factor
    of exactly 0.01 is therefore METALLIC upstream. 0.0099999997 (below the float literal) stays diffuse."""
    import struct
    blob = struct.pack("<9f", 0, 0, 0, 1, 0, 0, 0, 1, 0) + struct.pack("<9f", 0, 0, 1, 0, 0, 1, 0, 0, 1) + struct.pack("<6f", 0, 0, 1, 0, 0, 1) + struct.pack("<3H", 0, 1, 2) + b"\0\0"
    for factor, exp in ((0.01, abi.RT_MAT_METALLIC), (0.0099999997, abi.RT_MAT_DIFFUSE), (0.0, abi.RT_MAT_DIFFUSE), (1.0, abi.RT_MAT_METALLIC)):
        d = {"asset": {"version": "2.0"}, "buffers": [{"byteLength": len(blob)}],
             "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 36}, {"buffer": 0, "byteOffset": 36, "byteLength": 36},
                             {"buffer": 0, "byteOffset": 72, "byteLength": 24}, {"buffer": 0, "byteOffset": 96, "byteLength": 6}],
             "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"}, {"bufferView": 1, "componentType": 5126, "count": 3, "type": "VEC3"},
                           {"bufferView": 2, "componentType": 5126, "count": 3, "type": "VEC2"}, {"bufferView": 3, "componentType": 5123, "count": 3, "type": "SCALAR"}],
             "materials": [{"pbrMetallicRoughness": {"metallicFactor": factor}}],
             "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2}, "indices": 3, "material": 0}]}],
             "nodes": [{"mesh": 0}], "scenes": [{"nodes": [0]}], "scene": 0}
        pth = tmp_path / f"m_{factor}.glb"
        _craft_glb(pth, d, blob)
        cs = CppScene(hostlib, pth)
        assert cs.materials[0].type == exp, factor


def test_png_codec_against_pil(hostlib, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    path = tmp_path / "x.png"
    assert hostlib.rth_write_png(str(path).encode(), 53, 37, abi.u8ptr(np.ascontiguousarray(img))) == 0
    np.testing.assert_array_equal(np.asarray(Image.open(path).convert("RGBA")), img)  # our encoder, PIL's decoder
    for mode, ref in (("RGBA", img), ("RGB", img[..., :3]), ("L", img[..., 0]), ("P", None), ("LA", img[..., [0, 3]])):
        p = tmp_path / f"m_{mode}.png"
        pil = Image.fromarray(img, "RGBA").convert(mode) if mode != "LA" else Image.fromarray(np.ascontiguousarray(ref), "LA")
        pil.save(p)
        data = np.frombuffer(p.read_bytes(), np.uint8)
        w, h = C.c_uint32(), C.c_uint32()
        out = np.zeros((37, 53, 4), np.uint8)
        assert hostlib.rth_decode_png(abi.u8ptr(data), data.size, C.byref(w), C.byref(h), abi.u8ptr(out), out.size) == 0, \
            hostlib.rth_last_error()
        assert (w.value, h.value) == (53, 37)
        np.testing.assert_array_equal(out, np.asarray(pil.convert("RGBA")))  # PIL's encoder, our decoder


def test_texture_resize_semantics(hostlib):
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, (512, 512, 4), dtype=np.uint8)
    out = np.zeros_like(src)
    hostlib.rth_resize_to_layer(abi.u8ptr(src), 512, 512, abi.u8ptr(out))
    np.testing.assert_array_equal(out, src)  # 512x512 passes through untouched
    flat = np.full((64, 32, 4), (200, 100, 50, 255), np.uint8)
    hostlib.rth_resize_to_layer(abi.u8ptr(flat), 32, 64, abi.u8ptr(out))
    assert (out == np.array([200, 100, 50, 255], np.uint8)).all()  # constant images stay constant (up-sampling)
    big = np.zeros((1024, 1024, 4), np.uint8)
    big[..., 3] = 255
    big[:, 512:, :3] = 255
    hostlib.rth_resize_to_layer(abi.u8ptr(big), 1024, 1024, abi.u8ptr(out))
    assert (out[:, :255, :3] == 0).all() and (out[:, 257:, :3] == 255).all()  # 2x2 box average keeps the edge sharp


def test_cli_flags_match_the_reference(rtlib):
    exe = HOST / "raytracer"
    assert exe.exists()
    out = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("-d,--max-depth", "-s,--sample-count", "-w,--wavefront", "-m,--megakernel", "scene_path", "--rr", "--devices"):
        assert flag in out.stdout
    bad = subprocess.run([str(exe), "--nope"], capture_output=True, text=True)
    assert bad.returncode != 0 and "not expected" in bad.stderr
    bad = subprocess.run([str(exe), "-d", "abc"], capture_output=True, text=True)
    assert bad.returncode != 0
    if rtlib.rt_device_count() <= 0:  # no GPU here: the CLI must fail loudly, not fall back
        r = subprocess.run([str(exe), "-s", "1", str(REPO / "assets" / "cube.glb")], capture_output=True, text=True)
        assert r.returncode != 0 and "no HIP device" in r.stdout


def test_python_mirror_loads_glb_through_the_cpp_loader(oracle, scene_cache, tmp_path):
    """rtamd.loader.load_glb (the C++ loader behind the Python mirror): the shipped assets give the SceneDesc of the
    pure-Python reader, and a textured, instanced scene survives export -> load with an identical render."""
    from rtamd import loader
    for name in ("triangle", "cube"):
        a, b = loader.load_glb(REPO / "assets" / f"{name}.glb"), scene_cache(name)
        for f in ("positions", "normals", "uvs", "indices", "tri_instance", "transforms", "normal_mats", "inst_material", "sky"):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
        assert [(m.type, m.tex_layer) for m in a.materials] == [(m.type, m.tex_layer) for m in b.materials]
    sd = scene_cache("atrium", detail=1)
    export_glb(sd, tmp_path / "a.glb", jpeg_quality=None)
    ld = loader.load_glb(tmp_path / "a.glb")
    assert ld.n_triangles == sd.n_triangles and ld.textures.shape == sd.textures.shape
    np.testing.assert_array_equal(ld.textures, sd.textures)
    cam = oracle.camera(40, 24, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    fa, _, ra = oracle.OracleScene(sd).render(cam, 0, 5, 2)
    fb, _, rb = oracle.OracleScene(ld).render(cam, 0, 5, 2)
    assert ra == rb
    np.testing.assert_array_equal(fa, fb)


def test_node_globals_are_composed_from_the_node_up_and_the_camera_through_a_quaternion(hostlib, tmp_path):
    """VERDICT r4 item 4. The reference composes a node's global matrix from the node UP (src/scene.cpp:137-146: m = local * scale(global_scale);
    m = ancestor.local * m, nearest ancestor first) and turns (0, 0, -1) by quat_cast(global) for the camera direction (:113-121). fp32 matrix
    products do not associate, so a hierarchy three deep with rotations and non-uniform scales tells the two composition orders apart in the low
    bits: both loaders (C++ and Python) must carry the bottom-up bits, equal to each other, and differ from the top-down product. Under a scaled
    camera chain the quaternion direction is not minus the matrix's third column."""
    import struct
    from rtamd.scenes import camera_direction_of, load_glb, mat4_identity, mat4_mul, mat4_scale, trs
    blob = struct.pack("<9f", 0, 0, 0, 1, 0, 0, 0, 1, 0) + struct.pack("<9f", 0, 0, 1, 0, 0, 1, 0, 0, 1) + struct.pack("<6f", 0, 0, 1, 0, 0, 1) + struct.pack("<3H", 0, 1, 2) + b"\0\0"
    def quat(axis, angle):
        a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
        return [float(v) for v in (*(a * np.sin(angle / 2)), np.cos(angle / 2))]
    nodes = [
        {"translation": [0.37, -1.21, 2.05], "rotation": quat((0.3, 1.0, 0.2), 0.58), "scale": [1.7, 0.9, 1.3], "children": [1, 4]},
        {"translation": [-0.61, 0.13, 0.77], "rotation": quat((1.0, 0.1, -0.4), 1.91), "scale": [0.8, 1.1, 2.3], "children": [2]},
        {"translation": [0.05, 0.5, -0.33], "rotation": quat((-0.2, 0.7, 0.6), 2.63), "scale": [1.9, 0.6, 0.7], "children": [3]},
        {"translation": [1.3, -0.4, 0.2], "rotation": quat((0.5, -0.5, 0.7), 0.91), "scale": [1.2, 1.2, 0.4], "mesh": 0},
        {"translation": [0.2, 0.1, -3.0], "rotation": quat((0.1, 0.9, 0.3), 1.27), "scale": [1.0, 2.5, 0.6], "children": [5]},
        {"translation": [0.0, 0.3, 0.1], "rotation": quat((0.8, 0.2, -0.1), 0.44), "camera": 0},
    ]
    d = {"asset": {"version": "2.0"}, "buffers": [{"byteLength": len(blob)}],
         "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 36}, {"buffer": 0, "byteOffset": 36, "byteLength": 36},
                         {"buffer": 0, "byteOffset": 72, "byteLength": 24}, {"buffer": 0, "byteOffset": 96, "byteLength": 6}],
         "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"}, {"bufferView": 1, "componentType": 5126, "count": 3, "type": "VEC3"},
                       {"bufferView": 2, "componentType": 5126, "count": 3, "type": "VEC2"}, {"bufferView": 3, "componentType": 5123, "count": 3, "type": "SCALAR"}],
         "materials": [{"pbrMetallicRoughness": {"metallicFactor": 0.0}}], "cameras": [{"type": "perspective", "perspective": {"yfov": 0.7, "znear": 0.1}}],
         "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2}, "indices": 3, "material": 0}]}],
         "nodes": nodes, "scenes": [{"nodes": [0]}], "scene": 0}
    pth = tmp_path / "deep.glb"
    _craft_glb(pth, d, blob)
    cs = CppScene(hostlib, pth)
    py = load_glb(pth, "deep")
    local = [trs(n.get("translation", (0, 0, 0)), n.get("rotation", (0, 0, 0, 1)), n.get("scale", (1, 1, 1))) for n in nodes]
    local = [mat4_mul(m, mat4_identity()) for m in local]
    bottom_up = mat4_mul(local[0], mat4_mul(local[1], mat4_mul(local[2], mat4_mul(local[3], mat4_scale((1, 1, 1))))))
    top_down = mat4_mul(mat4_mul(mat4_mul(local[0], local[1]), local[2]), local[3])
    assert (bottom_up.view(np.uint32) != top_down.view(np.uint32)).any(), "the test hierarchy does not tell the two orders apart"
    got_cpp = np.array(list(cs.instances[0].transform), np.float32)
    np.testing.assert_array_equal(got_cpp.view(np.uint32), bottom_up.view(np.uint32))
    np.testing.assert_array_equal(py.transforms[0].view(np.uint32), bottom_up.view(np.uint32))
    np.testing.assert_array_equal(np.array(list(cs.instances[0].normal_mat), np.float32).view(np.uint32), py.normal_mats[0].view(np.uint32))
    # the camera: node 5 under the scaled node 4 under the scaled node 0
    cam_global = mat4_mul(local[0], mat4_mul(local[4], mat4_mul(local[5], mat4_scale((1, 1, 1)))))
    want_dir = camera_direction_of(cam_global)
    assert cs.has_camera
    np.testing.assert_array_equal(np.array(cs.camera.direction, np.float32).view(np.uint32), np.array(want_dir, np.float32).view(np.uint32))
    np.testing.assert_array_equal(np.array(py.camera.direction, np.float32).view(np.uint32), np.array(want_dir, np.float32).view(np.uint32))
    np.testing.assert_array_equal(np.array(cs.camera.position, np.float32).view(np.uint32), cam_global[12:15].view(np.uint32))
    minus_z = -cam_global[8:11].astype(np.float64); minus_z /= np.linalg.norm(minus_z)
    assert np.abs(np.array(want_dir) - minus_z).max() > 1e-3  # a scaled chain: the rotation the quaternion extracts is not the matrix's third column
    assert abs(np.linalg.norm(want_dir) - 1.0) < 1e-6


def test_scene_rules_against_the_host_builder_under_asan_ubsan(tmp_path):
    """csrc/scene_rules.h, the one text of the scene's geometry rules, in a stand-alone host program (tests/tools/scene_rules_check.cpp) on a small
    random tree over two instances, for the builders whose unions are exact (LBVH, SAH without pre-split triangles). The world vertices, leaf
    records, record boxes, shading words and normals the rules give are flatten()'s bit for bit; refit_host and refit_node applied node by
    node reproduce words 0..11 of every built node and every leaf record on unchanged vertices; with every vertex moved each node's decoded
    child boxes contain their children's exact boxes. Host compiler of the library's build, -ffp-contract=off as there, AddressSanitizer + UBSan on the host code (the program has none for a device)."""
    csrc = REPO / "sycl-ray-tracer_amd" / "csrc"
    exe = tmp_path / "scene_rules_check"
    srcs = [str(REPO / "tests" / "tools" / "scene_rules_check.cpp"), str(csrc / "scene_build.cpp"), str(csrc / "scene_check.cpp")]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", f"-I{csrc}", f"-I{REPO / 'include'}", "-o", str(exe)] + srcs, check=True, capture_output=True)
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.split()[0] == "ok" and int(p.stdout.split()[1]) > 500, p.stdout

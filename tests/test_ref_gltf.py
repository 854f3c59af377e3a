"""The GLB loaders against the REFERENCE's own glTF parser (VERDICT "What's missing" item 3).

oracle/_ref/libref_gltf.so is the reference's vendored tinygltf (with its nlohmann json and stb_image), compiled where the reference's
sources are at hand (`make -C oracle ref`; recipe and wrapper oracle/ref_gltf.cpp in oracle/, binary git-ignored). The wrapper loads a
file exactly as src/scene.cpp:56-62 does and returns every field Scene::Scene, load_images, load_primitives and load_node take from the
tinygltf::Model, as named flat arrays; it does no glm arithmetic.

This module writes a deterministic set of small GLBs, each doing one thing a foreign exporter does and rtamd/glb_export.py does not
(GOOD), asks the reference for each — ret must be true, err empty and no undefined read flagged — and compares the result field by
field, floats by bit pattern, with host/scene_loader.cpp (rth_load_glb's rt_scene_desc) and with rtamd/scenes.py. A second, closed list
(CLOSED) holds the inputs on which the reference's behaviour is undefined or a refusal; DESIGN §2 states what the loaders do there, and
the tests assert exactly that.

Where the library was never built, the tests compare against what it returned for the same file bytes, stored in
tests/golden/ref_gltf/ref_gltf.npz under the SHA-256 of each file (tests/golden/make_ref_gltf.py). Where it is built, the stored
vectors are checked against it. Nothing here skips."""
import ctypes as C
import hashlib
import json
import os
import re
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.scenes import camera_direction_of, mat4_identity, mat4_mul, mat4_scale, normal_matrix, trs

REPO = Path(__file__).resolve().parent.parent
REF = REPO / "oracle" / "_ref" / "libref_gltf.so"
HOST = REPO / "sycl-ray-tracer_amd" / "host" / "build" / "librt_host.so"
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_gltf"
STORED = GOLDEN / "ref_gltf.npz"
RECORD_ENV = "RT_REF_GLTF_RECORD"  # set by tests/golden/make_ref_gltf.py: the file the live library's results are written to
f32 = np.float32
_DTYPES = {0: np.float32, 1: np.float64, 2: np.int64, 3: np.uint32, 4: np.uint8}


def bits(a) -> np.ndarray:
    """float32 values as their bit patterns: the comparisons below carry no tolerance, and tell -0 from +0"""
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------------------
# writing GLB files
# ----------------------------------------------------------------------------------------------------------------------------------
def glb_bytes(js, bin_chunk: bytes = b"", bin_tail: int = 0) -> bytes:
    """A GLB of one JSON chunk (a dict, or the literal JSON text as bytes) and one BIN chunk, `bin_tail` more zero bytes at its end.
    The same container as test_host_cpp._craft_glb, returned instead of written."""
    j = json.dumps(js).encode() if not isinstance(js, bytes) else js
    j += b" " * (-len(j) % 4)
    b = bin_chunk + b"\0" * (-len(bin_chunk) % 4) + b"\0" * bin_tail
    body = struct.pack("<II", len(j), 0x4E4F534A) + j + (struct.pack("<II", len(b), 0x004E4942) + b if b else b"")
    return struct.pack("<4sII", b"glTF", 2, 12 + len(body)) + body


def _unit(seed: int, *shape) -> np.ndarray:
    """deterministic values in [0, 1) from the scene generator's integer hash (no library RNG: the files must never change)"""
    n = int(np.prod(shape))
    return (scenes._hash2(np.arange(n), np.full(n, 7), seed).astype(np.float64) / 4294967296.0).reshape(shape)


def _soup(seed: int, n_vertices: int, n_triangles: int):
    """a vertex soup with distinct bytes everywhere: a read at a wrong offset or stride cannot go unnoticed"""
    P = (_unit(seed, n_vertices, 3) * 4 - 2).astype(f32)
    N = (_unit(seed + 1, n_vertices, 3) * 2 - 1).astype(f32)
    UV = _unit(seed + 2, n_vertices, 2).astype(f32)
    I = (_unit(seed + 3, n_triangles, 3) * n_vertices).astype(np.uint32)
    return P, N, UV, I


def _png(img: np.ndarray, depth16: bool = False) -> bytes:
    """An (h, w, c) uint8 image (c = 3 RGB, 4 RGBA) as a PNG, written by hand with stored deflate blocks so that the bytes depend on no
    library version. depth16: every sample s becomes the 16-bit sample (s << 8) | (s * 7 % 256)."""
    h, w, c = img.shape
    rows = img.reshape(h, w * c)
    if depth16:
        rows = np.stack([rows, (rows.astype(np.int32) * 7 % 256).astype(np.uint8)], -1).reshape(h, -1)
    raw = b"".join(b"\0" + r.tobytes() for r in rows)
    assert len(raw) < 65536
    z = b"\x78\x01" + b"\x01" + struct.pack("<HH", len(raw), len(raw) ^ 0xFFFF) + raw + struct.pack(">I", zlib.adler32(raw))
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    ihdr = struct.pack(">IIBBBBB", w, h, 16 if depth16 else 8, {3: 2, 4: 6}[c], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", z) + chunk(b"IEND", b"")


def _picture(seed: int, h: int, w: int, c: int = 4) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 16 + 7 * seed) % 256, (y * 13 + 40) % 256, ((x // 4 + y // 4) % 2) * 200 + 30, 255 - (x + y) % 3], -1)
    return np.ascontiguousarray(img[..., :c].astype(np.uint8))


JPEG16 = (GOLDEN / "tex16.jpg").read_bytes()  # a 16 x 16 baseline 4:2:0 JPEG (a data fixture: no JPEG encoder is restated here)


class Bin:
    """The BIN chunk under construction, with its bufferViews and accessors."""

    def __init__(self):
        self.b, self.views, self.accs = bytearray(), [], []

    def view(self, data: bytes, stride: int | None = None, lead: int = 0) -> int:
        self.b += b"\xAB" * (-len(self.b) % 4 + lead)  # `lead` junk bytes in front of the view: a byteOffset that must not be dropped
        v = {"buffer": 0, "byteOffset": len(self.b), "byteLength": len(data)}
        if not len(self.b):
            del v["byteOffset"]  # absent = 0
        if stride is not None:
            v["byteStride"] = stride
        self.b += data
        self.views.append(v)
        return len(self.views) - 1

    def acc(self, view: int, ctype: int, count: int, typ: str, offset: int | None = None, **kw) -> int:
        a = {"bufferView": view, "componentType": ctype, "count": int(count), "type": typ, **kw}
        if offset is not None:
            a["byteOffset"] = offset
        self.accs.append(a)
        return len(self.accs) - 1

    def packed(self, P, N, UV, I, itype=np.uint16, material: int | None = 0) -> dict:
        """one tightly packed view per attribute, as glb_export writes them (but with `itype` indices)"""
        at = {"POSITION": self.acc(self.view(P.astype(f32).tobytes()), 5126, len(P), "VEC3"),
              "NORMAL": self.acc(self.view(N.astype(f32).tobytes()), 5126, len(N), "VEC3"),
              "TEXCOORD_0": self.acc(self.view(UV.astype(f32).tobytes()), 5126, len(UV), "VEC2")}
        p = {"attributes": at, "indices": self.indices(I, itype)}
        if material is not None:
            p["material"] = material
        return p

    def indices(self, I, itype=np.uint16, lead: int = 0, offset: int | None = None) -> int:
        ctype = {np.uint8: 5121, np.uint16: 5123, np.uint32: 5125}[itype]
        data = b"\xCD" * (offset or 0) + np.asarray(I).astype(itype).tobytes()
        return self.acc(self.view(data, lead=lead), ctype, np.asarray(I).size, "SCALAR", offset)

    def interleaved(self, P, N, UV, stride: int) -> dict:
        """position | normal | uv in one view, `stride` bytes per vertex (32 = no padding), junk in the padding"""
        rows = np.full((len(P), stride), 0xEE, np.uint8)
        rows[:, 0:12] = np.ascontiguousarray(P, f32).view(np.uint8).reshape(len(P), 12)
        rows[:, 12:24] = np.ascontiguousarray(N, f32).view(np.uint8).reshape(len(P), 12)
        rows[:, 24:32] = np.ascontiguousarray(UV, f32).view(np.uint8).reshape(len(P), 8)
        v = self.view(rows.tobytes(), stride)
        return {"POSITION": self.acc(v, 5126, len(P), "VEC3"), "NORMAL": self.acc(v, 5126, len(P), "VEC3", 12),
                "TEXCOORD_0": self.acc(v, 5126, len(P), "VEC2", 24)}

    def doc(self, **sections) -> dict:
        d = {"asset": {"version": "2.0"}, "buffers": [{"byteLength": len(self.b)}], "bufferViews": self.views, "accessors": self.accs}
        d.update(sections)
        return d


CAMERA = [{"type": "perspective", "perspective": {"yfov": 0.7, "znear": 0.1, "aspectRatio": 1.5}}]


def _simple(B: Bin, prims, materials=None, **over) -> dict:
    """one mesh on node 0, the camera on node 1 (the reference does not take a camera on node 0: CLOSED), one scene"""
    d = B.doc(meshes=[{"primitives": prims}], nodes=[{"mesh": 0}, {"camera": 0, "translation": [0, 0, 5]}], cameras=CAMERA,
              scenes=[{"nodes": [0, 1]}], scene=0)
    if materials is not None:
        d["materials"] = materials
    d.update(over)
    return d


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return [float(v) for v in (*(a * np.sin(angle / 2)), np.cos(angle / 2))]


def _rot_scale_matrix(axis, angle, s, t):
    """a column-major 4x4 of a rotation, a scale and a translation, as an exporter writes a `matrix` node (float64 numbers)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    M = np.eye(4)
    M[:3, :3] = R @ np.diag(s)
    M[:3, 3] = t
    return [float(v) for v in M.T.reshape(-1)]


# ---- GOOD: the reference loads each of these with ret = true, no error and no undefined read ----
def file_interleaved_32():
    B = Bin()
    P, N, UV, I = _soup(11, 37, 23)
    return glb_bytes(_simple(B, [{"attributes": B.interleaved(P, N, UV, 32), "indices": B.indices(I), "material": 0}], [{}]), bytes(B.b))


def file_interleaved_48():
    B = Bin()
    P, N, UV, I = _soup(12, 41, 19)
    return glb_bytes(_simple(B, [{"attributes": B.interleaved(P, N, UV, 48), "indices": B.indices(I), "material": 0}], [{}]), bytes(B.b))


def file_stride_equal_to_packed():
    """byteStride present but equal to the element size (12 / 12 / 8): ByteStride() returns it, the reference divides it by 4"""
    B = Bin()
    P, N, UV, I = _soup(13, 29, 17)
    at = {"POSITION": B.acc(B.view(P.tobytes(), 12), 5126, len(P), "VEC3"), "NORMAL": B.acc(B.view(N.tobytes(), 12), 5126, len(N), "VEC3"),
          "TEXCOORD_0": B.acc(B.view(UV.tobytes(), 8), 5126, len(UV), "VEC2")}
    return glb_bytes(_simple(B, [{"attributes": at, "indices": B.indices(I), "material": 0}], [{}]), bytes(B.b))


def file_offsets():
    """accessor byteOffset and view byteOffset both non-zero (attributes and indices), views listed in another order than the accessors
    that use them, and a BIN chunk longer than buffers[0].byteLength"""
    B = Bin()
    P, N, UV, I = _soup(14, 33, 21)
    junk = lambda n, c: bytes([c]) * n
    vp = B.view(junk(24, 0x11) + P.tobytes(), lead=8)
    vn = B.view(junk(12, 0x22) + N.tobytes(), lead=4)
    vt = B.view(junk(40, 0x33) + UV.tobytes(), lead=12)
    at = {"POSITION": B.acc(vp, 5126, len(P), "VEC3", 24), "NORMAL": B.acc(vn, 5126, len(N), "VEC3", 12), "TEXCOORD_0": B.acc(vt, 5126, len(UV), "VEC2", 40)}
    d = _simple(B, [{"attributes": at, "indices": B.indices(I, np.uint16, lead=6, offset=10), "material": 0}], [{}])
    perm = [2, 0, 3, 1]  # new position of each view
    d["bufferViews"] = [B.views[perm.index(k)] for k in range(4)]
    for a in d["accessors"]:
        a["bufferView"] = perm[a["bufferView"]]
    return glb_bytes(d, bytes(B.b), bin_tail=12)


def file_index_types():
    B = Bin()
    prims = []
    for k, (itype, nv) in enumerate(((np.uint8, 200), (np.uint16, 300), (np.uint32, 300))):
        P, N, UV, I = _soup(20 + 4 * k, nv, 31)
        I[0] = [nv - 1, 0, nv - 2]  # the largest index of each width's file is used
        prims.append(B.packed(P, N, UV, I, itype))
    return glb_bytes(_simple(B, prims, [{}]), bytes(B.b))


def file_index_view_with_stride():
    """a byteStride on the index view: tinygltf takes it, the reference reads the indices packed all the same (src/scene.cpp:375-395)"""
    B = Bin()
    P, N, UV, I = _soup(15, 50, 13)
    p = B.packed(P, N, UV, I, np.uint32)
    v = B.accs[p["indices"]]["bufferView"]
    B.views[v]["byteStride"] = 8
    B.b += b"\x05" * (I.size * 4 + 8)  # room for a strided read, so that no loader can refuse the file for its size
    return glb_bytes(_simple(B, [p], [{}]), bytes(B.b))


def _box_parts():
    P, N, UV, I = scenes.mesh_box()
    return P.astype(f32), N.astype(f32), UV.astype(f32), I.astype(np.uint32)


def file_hierarchy():
    """several primitives per mesh with different materials (sharing their vertex accessors), one mesh used by several nodes, a node
    with a mesh AND children, a hierarchy four deep mixing a `matrix` node with TRS nodes that have only some of T, R, S, and a node no
    scene reaches. Rendered by the GPU check."""
    B = Bin()
    P, N, UV, I = _box_parts()
    at = B.packed(P, N, UV, I[:4], np.uint8, 0)
    box = [at, {"attributes": at["attributes"], "indices": B.indices(I[4:8], np.uint16), "material": 1},
           {"attributes": at["attributes"], "indices": B.indices(I[8:], np.uint32), "material": 2}]
    fp, fn, fuv, fi = scenes.mesh_quad((-5, 0, 5), (5, 0, 5), (5, 0, -5), (-5, 0, -5), 3, 3)
    floor = [B.packed(fp, fn, fuv, fi, np.uint16, 3)]
    materials = [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.2, 0.15, 1.0], "metallicFactor": 0.0}},
                 {"pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.8, 0.5, 1.0], "metallicFactor": 1.0, "roughnessFactor": 0.25}},
                 {"pbrMetallicRoughness": {"metallicFactor": 0}, "emissiveFactor": [1.0, 0.8, 0.5], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 4.0}}},
                 {"pbrMetallicRoughness": {"baseColorFactor": [0.6, 0.65, 0.7, 1.0], "metallicFactor": 0.0}}]
    nodes = [{"translation": [0.2, 0.0, -0.5], "children": [1, 4], "mesh": 1},
             {"matrix": _rot_scale_matrix((0.2, 1.0, 0.1), 0.6, (0.9, 0.7, 0.8), (-1.6, 0.9, 0.3)), "children": [2]},
             {"rotation": _quat((1.0, 0.3, -0.2), 0.8), "scale": [0.9, 1.2, 0.7], "mesh": 0, "children": [3]},
             {"scale": [0.5, 0.5, 1.4], "translation": [1.1, 1.9, 0.4], "mesh": 0},
             {"rotation": _quat((0.1, 1.0, 0.3), -0.7), "translation": [2.1, 0.8, 0.6], "mesh": 0},
             {"translation": [0.3, 2.2, 7.5], "rotation": _quat((1, 0, 0), -0.2), "camera": 0},
             {"mesh": 0, "translation": [0, 1, 3]}]  # reached by no scene
    d = B.doc(meshes=[{"primitives": box}, {"primitives": floor}], nodes=nodes, materials=materials, cameras=CAMERA,
              scenes=[{"nodes": [0, 5], "extras": {"sky_color": [0.6, 0.7, 0.9], "sky_strength": 1.5}}], scene=0)
    return glb_bytes(d, bytes(B.b))


def file_interleaved_textured():
    """an interleaved box of two primitives with a PNG-textured diffuse and a JPEG-textured metallic material, a textured floor, rotated
    instances; textures[].source is not the identity. Rendered by the GPU check."""
    B = Bin()
    P, N, UV, I = _box_parts()
    at = B.interleaved(P, N, UV, 32)
    box = [{"attributes": at, "indices": B.indices(I[:6], np.uint16), "material": 0}, {"attributes": at, "indices": B.indices(I[6:], np.uint8), "material": 1}]
    fp, fn, fuv, fi = scenes.mesh_quad((-5, 0, 5), (5, 0, 5), (5, 0, -5), (-5, 0, -5), 2, 2, (4, 4))
    floor = [{"attributes": B.interleaved(fp, fn, fuv, 48), "indices": B.indices(fi, np.uint32), "material": 2}]
    imgs = [B.view(_png(_picture(1, 16, 16, 4))), B.view(JPEG16), B.view(_png(_picture(3, 8, 12, 3)))]
    images = [{"bufferView": imgs[0], "mimeType": "image/png"}, {"bufferView": imgs[1], "mimeType": "image/jpeg"}, {"bufferView": imgs[2], "mimeType": "image/png"}]
    textures = [{"source": 1}, {"source": 2}, {"source": 0}]
    tex = lambda i: {"index": i}
    materials = [{"pbrMetallicRoughness": {"baseColorTexture": tex(2), "metallicFactor": 0.0}},
                 {"pbrMetallicRoughness": {"baseColorTexture": tex(0), "metallicFactor": 0.9, "roughnessFactor": 0.3}},
                 {"pbrMetallicRoughness": {"baseColorTexture": tex(1), "metallicFactor": 0.0}}]
    nodes = [{"mesh": 1}, {"mesh": 0, "translation": [-1.3, 1.0, 0.0], "rotation": _quat((0.2, 1.0, 0.0), 0.7)},
             {"mesh": 0, "translation": [1.4, 0.8, -0.6], "rotation": _quat((1.0, 0.4, 0.3), 1.1), "scale": [0.8, 0.8, 0.8]},
             {"translation": [0.0, 2.0, 7.0], "rotation": _quat((1, 0, 0), -0.15), "camera": 0}]
    d = B.doc(meshes=[{"primitives": box}, {"primitives": floor}], nodes=nodes, materials=materials, cameras=CAMERA, images=images, textures=textures,
              scenes=[{"nodes": [0, 1, 2, 3], "extras": {"sky_color": [0.9, 0.9, 1.0]}}], scene=0)
    return glb_bytes(d, bytes(B.b))


def _two_scenes(with_scene: bool):
    B = Bin()
    P, N, UV, I = _soup(30, 24, 11)
    P2, N2, UV2, I2 = _soup(34, 18, 9)
    d = B.doc(meshes=[{"primitives": [B.packed(P, N, UV, I)]}, {"primitives": [B.packed(P2, N2, UV2, I2, material=1)]}],
              materials=[{"pbrMetallicRoughness": {"metallicFactor": 0.0}}, {}], cameras=CAMERA,
              nodes=[{"mesh": 0}, {"mesh": 1, "translation": [1, 2, 3]}, {"camera": 0, "translation": [0, 0, 4]}, {"camera": 0, "translation": [0, 0, 9]},
                     {"mesh": 0, "scale": [2, 2, 2]}],  # node 4: in no scene
              scenes=[{"nodes": [0, 2], "extras": {"sky_color": [0.1, 0.2, 0.3]}}, {"nodes": [3, 1], "extras": {"sky_color": [0.4, 0.5, 0.6], "sky_strength": 2}}])
    if with_scene:
        d["scene"] = 1
    return glb_bytes(d, bytes(B.b))


def file_two_scenes_scene_1():
    return _two_scenes(True)


def file_two_scenes_scene_absent():
    return _two_scenes(False)


def file_numbers():
    """JSON numbers in every spelling an exporter may write, in node transforms and material factors. The text is literal: json.dumps
    would normalise the spellings away."""
    B = Bin()
    P, N, UV, I = _soup(40, 12, 5)
    prim, prim1 = B.packed(P, N, UV, I[:3]), B.packed(P, N, UV, I[3:], material=1)
    head = json.dumps(B.doc())[1:-1]
    text = "{" + head + """,
      "meshes": [{"primitives": [%s, %s]}], "cameras": %s, "scene": 0,
      "scenes": [{"nodes": [0, 1, 2, 3, 4], "extras": {"sky_color": [1, 0.5, 2.5E-1], "sky_strength": 2}}],
      "materials": [{"pbrMetallicRoughness": {"baseColorFactor": [0.1, 1.0000000000000002, 1e-3, 1], "metallicFactor": 5e-324, "roughnessFactor": 1E+2},
                     "emissiveFactor": [16777217, 0.30000000000000004, 12345678901234567890],
                     "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 1}}},
                    {"pbrMetallicRoughness": {"baseColorFactor": [-0, -0.0, -0e0, 1], "metallicFactor": 1E+2, "roughnessFactor": -0},
                     "emissiveFactor": [-0, -0.0, 5e-324], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 1}}}],
      "nodes": [{"mesh": 0, "translation": [1E+2, 1e-3, -0]},
                {"mesh": 0, "translation": [-0.0, 0.1, 1.0000000000000002], "scale": [16777217, 12345678901234567890, 1e-3]},
                {"mesh": 0, "translation": [5e-324, -0, 16777217], "scale": [1E+2, 0.1, 1e-3], "rotation": [-0, -0.0, 0.1, 1e-3]},
                {"mesh": 0, "matrix": [1E+2, -0, -0.0, 0, 1e-3, 0.1, 5e-324, 0, -0, 16777217, 1.0000000000000002, 0, 12345678901234567890, -0.0, -0, 1]},
                {"camera": 0, "translation": [0, 0, 5.0e0]}]}""" % (json.dumps(prim), json.dumps(prim1), json.dumps(CAMERA))
    return glb_bytes(text.encode(), bytes(B.b))


def file_json_text():
    """string escapes and \\u pairs in names, nested extras, unknown extensions, and whitespace / key order unlike json.dumps"""
    B = Bin()
    P, N, UV, I = _soup(44, 12, 5)
    prim = B.packed(P, N, UV, I)
    text = """\t{ "scene"\r\n:\t0 ,"scenes":[ {"extras":{"nested":{"deeper":[1,[2,{"k":null}],true,false]},"sky_strength" : 0.5 ,
      "sky_color":[ 0.25,\n0.5 ,0.75 ] , "note":"tab\\there \\"quoted\\" back\\\\slash \\/ \\b\\f\\n\\r"} ,"nodes" :[1,0],"name":"sc\\u00e8ne \\ud83d\\ude00 \\u4e2d"}] ,
      "extensionsUsed":["VENDOR_unknown_thing"],
      "nodes":[{"name":"m\\u0065sh \\"node\\"","extensions":{"VENDOR_unknown_thing":{"a":[1,2,3],"b":{"c":"d"}}},"mesh":0,"extras":{"x":{"y":{"z":[]}}}} ,
               {"translation":[0,0,5],"camera":0,"name":"\\ud83c\\udfa5"}],
      "cameras":%s,"materials":[{"name":"mat\\u00e9riau","extras":[[[]]],"extensions":{"VENDOR_unknown_thing":{}} ,"pbrMetallicRoughness":{"roughnessFactor":0.5 ,"metallicFactor":1}}],
      "meshes":[{"primitives":[%s],"name":"\\u00fc"}],
      "accessors":%s , "bufferViews":%s,"buffers":[{"byteLength":%d}]
      ,"asset":{"generator":"by hand","version":"2.0"}  }\n""" % (json.dumps(CAMERA), json.dumps(prim), json.dumps(B.accs), json.dumps(B.views), len(B.b))
    return glb_bytes(text.encode(), bytes(B.b))


def _materials_file(seed, materials, **over):
    B = Bin()
    P, N, UV, I = _soup(seed, 12, 2 * len(materials))
    prims = [B.packed(P, N, UV, I[2 * k: 2 * k + 2], material=k) for k in range(len(materials))]
    return glb_bytes(_simple(B, prims, materials, **over), bytes(B.b))


def file_material_defaults():
    """every optional field absent: tiny_gltf.h's defaults (base colour 1, metallic 1, roughness 1, emissive 0)"""
    return _materials_file(50, [{}, {"pbrMetallicRoughness": {}}, {"name": "only a name"}, {"pbrMetallicRoughness": {"baseColorFactor": [0.5, 0.25, 0.125, 1]}}])


def file_metallic_threshold():
    """metallicFactor at 0.01, at its two double neighbours, and at float32(0.01) written out as a decimal: the reference compares the
    double with the float literal 0.01f (src/scene.cpp:219)"""
    lo, hi = np.nextafter(0.01, 0.0), np.nextafter(0.01, 1.0)
    text = [repr(0.01), repr(float(lo)), repr(float(hi)), "0.00999999977648258209228515625", repr(float(np.nextafter(np.float64(f32(0.01)), 1.0))),
            repr(float(np.nextafter(np.float64(f32(0.01)), 0.0)))]
    raw = _materials_file(52, [{"pbrMetallicRoughness": {"metallicFactor": f"@{k}@"}} for k in range(len(text))])
    # the factors go in as literal text (the 29-digit decimal would not survive json.dumps); same length bookkeeping as glb_bytes
    jlen = struct.unpack_from("<I", raw, 12)[0]
    js, rest = raw[20:20 + jlen].decode().rstrip(" "), raw[20 + jlen:]
    for k, t in enumerate(text):
        js = js.replace(f'"@{k}@"', t)
    j = js.encode() + b" " * (-len(js.encode()) % 4)
    body = struct.pack("<II", len(j), 0x4E4F534A) + j + rest
    return struct.pack("<4sII", b"glTF", 2, 12 + len(body)) + body


def file_emissive():
    """emissiveFactor without the strength extension (the reference multiplies by 0), with it as an integer, as a float, and the extension
    present without its number"""
    ext = lambda v: {"KHR_materials_emissive_strength": v}
    return _materials_file(54, [{"emissiveFactor": [1.0, 0.5, 0.25]}, {"emissiveFactor": [1.0, 0.5, 0.25], "extensions": ext({"emissiveStrength": 3})},
                                {"emissiveFactor": [0.1, 0.7, 0.3], "extensions": ext({"emissiveStrength": 2.7})},
                                {"emissiveFactor": [1.0, 0.5, 0.25], "extensions": ext({})}, {"extensions": ext({"emissiveStrength": 5.0})}])


def file_ior_transmission():
    """ior without transmission and the reverse (neither is a dielectric), both, and both with the ior number absent (Value::Get of a missing
    key is a null Value, whose GetNumberAsDouble is 0)"""
    m = {"pbrMetallicRoughness": {"metallicFactor": 0.0, "baseColorFactor": [0.2, 0.4, 0.6, 1]}}
    return _materials_file(56, [{**m, "extensions": {"KHR_materials_ior": {"ior": 1.33}}}, {**m, "extensions": {"KHR_materials_transmission": {"transmissionFactor": 1}}},
                                {**m, "extensions": {"KHR_materials_ior": {"ior": 1.7}, "KHR_materials_transmission": {"transmissionFactor": 0.5}}},
                                {**m, "extensions": {"KHR_materials_ior": {"ior": 2}, "KHR_materials_transmission": {}}},
                                {**m, "extensions": {"KHR_materials_ior": {}, "KHR_materials_transmission": {}}}])


def file_texture_permutations():
    """baseColorTexture.index and textures[].source are different permutations; PNG (RGBA, RGB) and JPEG images in buffer views; a
    KHR_texture_transform the reference ignores; a dielectric with a texture it never looks at"""
    B = Bin()
    P, N, UV, I = _soup(58, 12, 8)
    imgs = [B.view(_png(_picture(5, 16, 16, 4))), B.view(JPEG16), B.view(_png(_picture(7, 5, 9, 3)))]
    images = [{"bufferView": v, "mimeType": t} for v, t in zip(imgs, ("image/png", "image/jpeg", "image/png"))]
    textures = [{"source": 2}, {"source": 0, "sampler": 0}, {"source": 1}]
    tex = lambda i, **kw: {"baseColorTexture": {"index": i, **kw}}
    materials = [{"pbrMetallicRoughness": {**tex(1), "metallicFactor": 0.0}}, {"pbrMetallicRoughness": {**tex(2), "metallicFactor": 1.0}},
                 {"pbrMetallicRoughness": {**tex(0, texCoord=0, extensions={"KHR_texture_transform": {"offset": [0.5, 0.25], "scale": [2, 2], "rotation": 0.3}}), "metallicFactor": 0}},
                 {"pbrMetallicRoughness": tex(1), "extensions": {"KHR_materials_ior": {"ior": 1.4}, "KHR_materials_transmission": {"transmissionFactor": 1}}}]
    prims = [B.packed(P, N, UV, I[2 * k: 2 * k + 2], material=k) for k in range(4)]
    d = _simple(B, prims, materials, images=images, textures=textures, samplers=[{}], extensionsUsed=["KHR_texture_transform"])
    return glb_bytes(d, bytes(B.b))


def file_cameras():
    """two cameras: the reference keeps the LAST camera node it visits (a node before its children, roots in the scene's order), here node 2
    under a rotated and scaled parent although node 4 has the larger index; aspectRatio absent; the first camera's yfov differs. At yfov
    0.305 the reference's float focal length, 1.0f / tanf(yfov / 2.0f), is not the double formula's rounded to float."""
    B = Bin()
    P, N, UV, I = _soup(60, 12, 4)
    cams = [{"type": "perspective", "perspective": {"yfov": 0.5, "znear": 0.1}}, {"type": "perspective", "perspective": {"yfov": 0.305, "znear": 0.01, "zfar": 100}}]
    nodes = [{"mesh": 0}, {"translation": [1, 2, 3], "rotation": _quat((0.3, 1, 0.2), 0.9), "scale": [1.5, 0.7, 2.0], "children": [2]},
             {"camera": 1, "translation": [0.1, 0.2, 0.3], "rotation": _quat((1, 0.2, 0), 0.4)}, {"children": [4]}, {"camera": 0, "translation": [0, 0, 5]}]
    d = B.doc(meshes=[{"primitives": [B.packed(P, N, UV, I)]}], nodes=nodes, materials=[{}], cameras=cams, scenes=[{"nodes": [3, 0, 1]}], scene=0)
    return glb_bytes(d, bytes(B.b))


def file_matrix_and_trs():
    """a node with `matrix` AND translation / rotation / scale (not valid glTF, and still written): tinygltf's ParseNode reads T / R / S only
    where `matrix` is absent or no array of numbers, so the reference sees the matrix alone"""
    B = Bin()
    P, N, UV, I = _soup(64, 9, 3)
    nodes = [{"mesh": 0, "matrix": _rot_scale_matrix((0, 1, 0.5), 0.4, (1, 2, 3), (4, 5, 6)), "translation": [9, 9, 9], "rotation": _quat((1, 0, 0), 1.0), "scale": [7, 7, 7]},
             {"camera": 0, "translation": [0, 0, 5]}, {"mesh": 0, "matrix": "none", "translation": [1, 2, 3]}]
    return glb_bytes(_simple(B, [B.packed(P, N, UV, I)], [{}], nodes=nodes, scenes=[{"nodes": [0, 1, 2]}]), bytes(B.b))


def _sky_file(extras):
    B = Bin()
    P, N, UV, I = _soup(62, 9, 3)
    return glb_bytes(_simple(B, [B.packed(P, N, UV, I)], [{}], scenes=[{"nodes": [0, 1], "extras": extras}]), bytes(B.b))


def file_sky_integer_spellings():
    return _sky_file({"sky_color": [1, 0, 2], "sky_strength": 3})


def file_sky_float_spellings():
    return _sky_file({"sky_color": [0.1, 0.30000000000000004, 1.0], "sky_strength": 0.7})


def file_sky_wrong_length():
    """a sky_color of four numbers is not taken (src/scene.cpp:80-81); the strength still multiplies the default sky (:90-92)"""
    return _sky_file({"sky_color": [0.1, 0.2, 0.3, 1.0], "sky_strength": 0.5})


def file_sky_not_numbers():
    return _sky_file({"sky_color": "blue", "sky_strength": "strong"})


def file_exported_cornell():
    """and one file of the project's own exporter (rtamd/glb_export.py: instancing, rotations, the emissive-strength / ior / transmission
    extensions, sky extras, a camera node), so that a misreading the exporter shares with the loaders shows too"""
    import tempfile
    from rtamd.glb_export import export_glb
    with tempfile.TemporaryDirectory() as d:
        export_glb(scenes.cornell_scene(), Path(d) / "cornell.glb")
        return (Path(d) / "cornell.glb").read_bytes()


GOOD = {f.__name__[5:]: f for f in (
    file_interleaved_32, file_interleaved_48, file_stride_equal_to_packed, file_offsets, file_index_types, file_index_view_with_stride, file_hierarchy,
    file_interleaved_textured, file_two_scenes_scene_1, file_two_scenes_scene_absent, file_numbers, file_json_text, file_material_defaults,
    file_metallic_threshold, file_emissive, file_ior_transmission, file_texture_permutations, file_cameras, file_sky_integer_spellings,
    file_sky_float_spellings, file_sky_wrong_length, file_sky_not_numbers, file_matrix_and_trs, file_exported_cornell)}
RENDERED = ("hierarchy", "interleaved_textured")  # the GPU check (tests/test_gpu_cli.py) renders these: their decoded image bytes are stored too


# ---- CLOSED: the reference's behaviour is undefined (its source reads what is not there) or tinygltf refuses the file. DESIGN §2 has the table. ----
def _closed_prim(**change):
    """the plain one-triangle-soup file with one thing about its primitive changed"""
    B = Bin()
    P, N, UV, I = _soup(70, 12, 4)
    p = B.packed(P, N, UV, I)
    materials = [{"pbrMetallicRoughness": {"metallicFactor": 0.0}}]
    for k, v in change.items():
        if k == "drop_attribute":
            del p["attributes"][v]
        elif k == "drop":
            del p[v]
        elif k == "normalized_uvs":
            uv16 = np.round(UV * 65535).astype(np.uint16)
            p["attributes"]["TEXCOORD_0"] = B.acc(B.view(uv16.tobytes()), 5123, len(UV), "VEC2", normalized=True)
        elif k == "sparse":
            a = B.accs[p["attributes"]["POSITION"]]
            a["sparse"] = {"count": 2, "indices": {"bufferView": B.view(np.array([1, 3], np.uint16).tobytes()), "componentType": 5123},
                           "values": {"bufferView": B.view(np.zeros((2, 3), f32).tobytes())}}
            if v == "no_view":
                del a["bufferView"]
    return glb_bytes(_simple(B, [p], materials), bytes(B.b))


def _closed_png16():
    B = Bin()
    P, N, UV, I = _soup(72, 12, 4)
    v = B.view(_png(_picture(9, 6, 10, 4), depth16=True))
    d = _simple(B, [B.packed(P, N, UV, I)], [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0}}],
                images=[{"bufferView": v, "mimeType": "image/png"}], textures=[{"source": 0}])
    return glb_bytes(d, bytes(B.b))


def _closed_camera(where):
    B = Bin()
    P, N, UV, I = _soup(74, 12, 4)
    nodes = {"node_0": [{"camera": 0, "translation": [1, 2, 3]}, {"mesh": 0}], "absent": [{"mesh": 0}, {"translation": [1, 2, 3]}]}[where]
    d = B.doc(meshes=[{"primitives": [B.packed(P, N, UV, I)]}], nodes=nodes, materials=[{}], cameras=CAMERA, scenes=[{"nodes": [0, 1]}], scene=0)
    return glb_bytes(d, bytes(B.b))


def _closed_container(what):
    good = file_interleaved_32()
    if what == "bad_magic":
        return b"glTG" + good[4:]
    if what == "length_past_the_file":
        return good[:8] + struct.pack("<I", len(good) + 4) + good[12:]
    if what == "bin_chunk_not_a_multiple_of_4":  # the chunk's length field says 2 bytes less; the header's total length follows it
        jlen = struct.unpack_from("<I", good, 12)[0]
        blen = struct.unpack_from("<I", good, 20 + jlen)[0]
        out = bytearray(good[:-2])
        struct.pack_into("<I", out, 20 + jlen, blen - 2)
        struct.pack_into("<I", out, 8, len(out))
        return bytes(out)
    if what == "buffer_longer_than_the_bin_chunk":
        jlen = struct.unpack_from("<I", good, 12)[0]
        d = json.loads(good[20:20 + jlen])
        d["buffers"][0]["byteLength"] += 64
        return glb_bytes(d, good[20 + jlen + 8:])
    B = Bin()
    P, N, UV, I = _soup(76, 12, 4)
    text = json.dumps(_simple(B, [B.packed(P, N, UV, I)], [{}]))
    text = {"json_trailing_comma": text[:-1] + ",}", "json_nan": text.replace('"yfov": 0.7', '"yfov": NaN'), "json_single_quotes": text.replace('"asset"', "'asset'"),
            "json_unterminated": text[:-1], "json_root_is_an_array": "[" + text + "]"}[what]
    return glb_bytes(text.encode(), bytes(B.b))


UNDEFINED = {  # name: (file, what the reference's wrapper must flag, what the C++ loader does: an error text, or None = loads)
    "no_normal": (lambda: _closed_prim(drop_attribute="NORMAL"), "no NORMAL", "glTF: primitives need POSITION, NORMAL, TEXCOORD_0 and indices"),
    "no_texcoord": (lambda: _closed_prim(drop_attribute="TEXCOORD_0"), "no TEXCOORD_0", "glTF: primitives need POSITION, NORMAL, TEXCOORD_0 and indices"),
    "no_indices": (lambda: _closed_prim(drop="indices"), "no indices", "glTF: primitives need POSITION, NORMAL, TEXCOORD_0 and indices"),
    "no_material": (lambda: _closed_prim(drop="material"), "no material: materials[-1]", None),
    "png_16_bit": (_closed_png16, "pixels are not width*height RGBA8", None),
    "normalized_uvs": (lambda: _closed_prim(normalized_uvs=True), "TEXCOORD_0 is not a plain float VEC2", "glTF: POSITION/NORMAL/TEXCOORD_0 must be float"),
    "sparse_accessor": (lambda: _closed_prim(sparse="with_view"), "POSITION is not a plain float VEC3", "glTF: sparse accessors are not supported"),
    "sparse_accessor_without_view": (lambda: _closed_prim(sparse="no_view"), "POSITION accessor without a bufferView", "glTF: sparse accessors are not supported"),
    "camera_on_node_0": (lambda: _closed_camera("node_0"), None, None),
    "no_camera": (lambda: _closed_camera("absent"), "no camera node", None),
}
REFUSED = {  # name: the text tinygltf's err must contain; the C++ loader's own error text
    "bad_magic": ("Invalid magic.", "not a GLB v2 file"),
    "length_past_the_file": ("Invalid glTF binary.", "GLB length runs past the end of the file"),
    "bin_chunk_not_a_multiple_of_4": ("BIN Chunk end is not aligned to a 4-byte boundary.", "BIN chunk length is not a multiple of 4"),
    "buffer_longer_than_the_bin_chunk": ("Invalid `byteLength'", "buffer is longer than the BIN chunk"),
    "json_trailing_comma": ("parse error", "JSON parse error"),
    "json_nan": ("parse error", "JSON parse error"),
    "json_single_quotes": ("parse error", "JSON parse error"),
    "json_unterminated": ("parse error", "JSON parse error"),
    "json_root_is_an_array": ("Root element is not a JSON object", "glTF: the JSON root is not an object"),
}


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference: live, or as stored
# ----------------------------------------------------------------------------------------------------------------------------------
class Reference:
    """What the reference's parser returns for a file: from oracle/_ref/libref_gltf.so, or from tests/golden/ref_gltf/ref_gltf.npz."""

    def __init__(self):
        self.lib = C.CDLL(str(REF)) if REF.exists() else None
        self.recording = bool(os.environ.get(RECORD_ENV))
        if self.recording and self.lib is None:
            raise RuntimeError(f"{RECORD_ENV} needs {REF} (make -C oracle ref)")
        if self.lib is not None:
            self.lib.ref_gltf_load.restype = C.c_void_p
            self.lib.ref_gltf_load.argtypes = [C.c_char_p]
            self.lib.ref_gltf_names.restype = C.c_char_p
            self.lib.ref_gltf_names.argtypes = [C.c_void_p]
            self.lib.ref_gltf_array.restype = C.c_void_p
            self.lib.ref_gltf_array.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
            self.lib.ref_gltf_free.argtypes = [C.c_void_p]
        self.stored, self.seen = {}, {}
        if STORED.exists() and not self.recording:
            with np.load(STORED) as z:  # one table of (file SHA-256 / field name, dtype, count) over one blob of bytes
                blob, at = z["blob"], 0
                for key, code, count in zip(z["keys"], z["dtypes"], z["counts"]):
                    sha, name = str(key).split("/", 1)
                    dtype = np.dtype(_DTYPES[int(code)])
                    self.stored.setdefault(sha, {})[name] = np.frombuffer(blob[at: at + int(count) * dtype.itemsize].tobytes(), dtype)
                    at += int(count) * dtype.itemsize

    def _live(self, path, keep_images: bool) -> dict:
        h = self.lib.ref_gltf_load(str(path).encode())
        try:
            out = {}
            for name in self.lib.ref_gltf_names(h).decode().split("\n"):
                if not name:
                    continue
                dt, n = C.c_int(), C.c_uint64()
                p = self.lib.ref_gltf_array(h, name.encode(), C.byref(dt), C.byref(n))
                dtype = np.dtype(_DTYPES[dt.value])
                out[name] = np.frombuffer(C.string_at(p, n.value * dtype.itemsize), dtype).copy() if n.value else np.zeros(0, dtype)
            for name in [k for k in out if re.fullmatch(r"image\.\d+\.bytes", k)]:  # image bytes are kept as digests (and whole for RENDERED)
                data = out[name] if keep_images else out.pop(name)
                out[name[:-5] + "sha256"] = np.frombuffer(hashlib.sha256(data.tobytes()).digest(), np.uint8).copy()
            return out
        finally:
            self.lib.ref_gltf_free(h)

    def load(self, data: bytes, tmp_path, keep_images: bool = False) -> dict:
        """the wrapper's named arrays for the file `data` (oracle/ref_gltf.cpp)"""
        sha = hashlib.sha256(data).hexdigest()
        if self.lib is None:
            assert sha in self.stored, "oracle/_ref/libref_gltf.so is not built and tests/golden/ref_gltf/ref_gltf.npz does not hold this file: " \
                                       "a crafted file changed without tests/golden/make_ref_gltf.py being run again"
            return self.stored[sha]
        path = Path(tmp_path) / f"{sha[:16]}.glb"
        path.write_bytes(data)
        out = self._live(path, keep_images)
        self.seen[sha] = out
        if not self.recording:  # the stored vectors are checked against the live library
            assert sha in self.stored, "tests/golden/ref_gltf/ref_gltf.npz does not hold this file: run tests/golden/make_ref_gltf.py"
            kept = self.stored[sha]
            assert sorted(kept) == sorted(out), f"stored fields differ from the reference's: {sorted(set(kept) ^ set(out))}"
            for name, v in out.items():
                assert kept[name].dtype == v.dtype and kept[name].tobytes() == v.tobytes(), f"tests/golden/ref_gltf/ref_gltf.npz disagrees with the reference on {name}"
        return out

    def save(self, path):
        codes = {np.dtype(v): k for k, v in _DTYPES.items()}
        rows = [(f"{sha}/{name}", v) for sha, fields in sorted(self.seen.items()) for name, v in sorted(fields.items())]
        np.savez_compressed(path, keys=np.array([k for k, _ in rows]), dtypes=np.array([codes[v.dtype] for _, v in rows], np.uint8),
                            counts=np.array([v.size for _, v in rows], np.int64), blob=np.frombuffer(b"".join(v.tobytes() for _, v in rows), np.uint8))


def text_of(ref: dict, name: str) -> str:
    return ref[name].tobytes().decode(errors="replace")


@pytest.fixture(scope="module")
def reference():
    ref = Reference()
    yield ref
    if ref.recording:
        ref.save(os.environ[RECORD_ENV])


def open_hostlib():
    """librt_host.so with the entry points this module and the GPU check of tests/test_gpu_cli.py use"""
    if not HOST.exists():
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(str(HOST))
    lib.rth_last_error.restype = C.c_char_p
    lib.rth_load_glb.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.rth_scene_free.argtypes = [C.c_void_p]
    lib.rth_scene_desc.argtypes = [C.c_void_p, C.POINTER(abi.rt_scene_desc)]
    lib.rth_scene_camera.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.rth_decode_image.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_size_t]
    lib.rth_resize_to_layer.argtypes = [C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]
    return lib


@pytest.fixture(scope="module")
def hostlib(rtlib):
    return open_hostlib()


@pytest.fixture(scope="module")
def files():
    """every crafted file, written once"""
    out = {name: f() for name, f in GOOD.items()}
    out.update({name: v[0]() for name, v in UNDEFINED.items()})
    out.update({name: _closed_container(name) for name in REFUSED})
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# the scene the reference's Scene::Scene builds from those fields (its glm arithmetic restated in numpy, as tests/test_host_cpp.py holds it)
# ----------------------------------------------------------------------------------------------------------------------------------
def _tanf(x):
    """the C library's float tangent: what `glm::tan(float)` is (src/scene.cpp:127)"""
    fn = C.CDLL(None).tanf
    fn.restype, fn.argtypes = C.c_float, [C.c_float]
    return f32(fn(float(x)))


class Expected:
    """The flat scene description that follows from the reference's fields: vertex data appended once per primitive in mesh order
    (load_primitives), one instance per primitive of every visited node with a mesh, in NODE INDEX order (src/scene.cpp:101-106), its
    transform composed from the node up (:137-146)."""

    def __init__(self, ref: dict):
        g = lambda k: ref[k]
        n_nodes = int(g("n_nodes")[0])
        local, parent = {}, {}
        for i in range(n_nodes):
            t, q, s, m = (g(f"node.{i}.{k}") for k in ("translation", "rotation", "scale", "matrix"))
            lm = trs(t if t.size == 3 else (0, 0, 0), q if q.size == 4 else (0, 0, 0, 1), s if s.size == 3 else (1, 1, 1))  # :458-466
            local[i] = mat4_mul(lm, m.astype(f32) if m.size == 16 else mat4_identity())                                   # :467-469, :18-21

        def walk(i, p):  # :450-476
            parent[i] = p
            for c in g(f"node.{i}.children"):
                walk(int(c), i)
        for r in g("scene_nodes"):
            walk(int(r), None)
        assert list(parent) == [int(v) for v in g("visit_order")]

        def global_of(i):  # :137-146
            m = mat4_mul(local[i], mat4_scale((1.0, 1.0, 1.0)))
            p = parent[i]
            while p is not None:
                m = mat4_mul(local[p], m)
                p = parent[p]
            return m
        self.global_of = global_of

        prim_count = [int(v) for v in g("mesh_primitives")]
        base, v0 = {}, 0
        pos, nrm, uv = [], [], []
        for mi, n in enumerate(prim_count):
            for pi in range(n):
                k = f"prim.{mi}.{pi}."
                base[mi, pi] = v0
                pos.append(g(k + "positions").reshape(-1, 3)), nrm.append(g(k + "normals").reshape(-1, 3)), uv.append(g(k + "uvs").reshape(-1, 2))
                v0 += pos[-1].shape[0]
        cat = lambda parts, w, dt: np.concatenate(parts) if parts else np.zeros((0, w), dt)
        self.positions, self.normals, self.uvs = cat(pos, 3, f32), cat(nrm, 3, f32), cat(uv, 2, f32)
        idx, tri_inst, self.transforms, self.normal_mats, self.inst_gltf_material = [], [], [], [], []
        for i in sorted(parent):
            mesh = int(g(f"node.{i}.mesh")[0])
            if mesh == -1:
                continue
            gm = global_of(i)
            for pi in range(prim_count[mesh]):
                k = f"prim.{mesh}.{pi}."
                tri = g(k + "indices").reshape(-1, 3) + np.uint32(base[mesh, pi])
                tri_inst.append(np.full(tri.shape[0], len(self.transforms), np.uint32))
                idx.append(tri)
                self.transforms.append(gm), self.normal_mats.append(normal_matrix(gm)), self.inst_gltf_material.append(int(g(k + "material")[0]))
        self.indices, self.tri_instance = cat(idx, 3, np.uint32), (np.concatenate(tri_inst) if tri_inst else np.zeros(0, np.uint32))
        self.n_images = int(g("n_images")[0])
        self.sky = np.array([0.5, 0.7, 1.0], f32)  # src/scene.hpp:76
        if "sky_color" in ref:
            self.sky = g("sky_color").copy()
        if "sky_strength" in ref:
            self.sky = (self.sky * g("sky_strength")[0]).astype(f32)
        self.ref = ref
        self.camera = None
        if "camera_yfov" in ref:
            cg = global_of(int(g("camera_node_index")[0]))
            yfov = g("camera_yfov")[0]
            self.camera = (cg[12:15].copy(), np.array(camera_direction_of(cg), f32), f32(f32(1.0) / _tanf(f32(yfov / f32(2.0)))))  # :113-127

    def material_record(self, gltf_index: int) -> bytes:
        """rt_material for a glTF material as the reference classifies it. The fields the reference's variant does not have take the
        ABI's fixed fill-ins: a dielectric is colour 0.8, roughness 0; a diffuse has roughness 0; the others' ior is 1.5."""
        g = lambda k: self.ref[f"material.{gltf_index}.{k}"]
        cls, image = int(g("class")[0]), int(g("image")[0])
        m = abi.rt_material()
        if cls == 2:
            m.type, m.tex_kind, m.ior = abi.RT_MAT_DIELECTRIC, abi.RT_TEX_COLOR, float(g("ior")[0])
            m.color[:] = [float(f32(0.8))] * 3
        else:
            m.type = abi.RT_MAT_METALLIC if cls == 1 else abi.RT_MAT_DIFFUSE
            m.tex_kind, m.tex_layer = (abi.RT_TEX_IMAGE, image) if image >= 0 else (abi.RT_TEX_COLOR, 0)
            m.color[:] = [float(v) for v in g("base_color")]
            m.emissive[:] = [float(v) for v in g("emissive")]
            m.roughness = float(g("roughness")[0]) if cls == 1 else 0.0
            m.ior = 1.5
        return bytes(m)

    def to_scene_desc(self, name: str, layers: np.ndarray) -> scenes.SceneDesc:
        """a SceneDesc for the oracle, materials indexed as the glTF file indexes them"""
        n_mat = int(self.ref["n_materials"][0])
        mats = []
        for i in range(n_mat):
            m = abi.rt_material.from_buffer_copy(self.material_record(i))
            mats.append(scenes.Material(int(m.type), tuple(m.color), int(m.tex_layer) if m.tex_kind == abi.RT_TEX_IMAGE else None, tuple(m.emissive), float(m.roughness), float(m.ior)))
        pos, dr, focal = self.camera
        return scenes.SceneDesc(name, self.positions, self.normals, self.uvs, self.indices, self.tri_instance, np.stack(self.transforms), np.stack(self.normal_mats),
                                np.asarray(self.inst_gltf_material, np.uint32), mats, layers, self.sky,
                                scenes.CameraPose(tuple(float(v) for v in pos), tuple(float(v) for v in dr), float(focal)))


def reference_images(ref: dict) -> list:
    """(h, w, 4) uint8 of every image the reference decoded (stored only for the RENDERED files)"""
    return [ref[f"image.{i}.bytes"].reshape(int(ref[f"image.{i}.height"][0]), int(ref[f"image.{i}.width"][0]), 4) for i in range(int(ref["n_images"][0]))]


def bake_layers(hostlib, images) -> np.ndarray:
    """512 x 512 layers of decoded images through the texture baker (pinned against the reference's resizer by tests/test_ref_stb.py)"""
    out = np.zeros((len(images), 512, 512, 4), np.uint8)
    for i, img in enumerate(images):
        img = np.ascontiguousarray(img)
        hostlib.rth_resize_to_layer(abi.u8ptr(img), img.shape[1], img.shape[0], abi.u8ptr(out[i]))
    return out


def embedded_images(data: bytes) -> list:
    """the undecoded bytes of every image of a GLB, cut out of its BIN chunk here"""
    jlen = struct.unpack_from("<I", data, 12)[0]
    js = json.loads(data[20:20 + jlen])
    bin0 = 20 + jlen + 8
    views = [js["bufferViews"][im["bufferView"]] for im in js.get("images", [])]
    return [data[bin0 + v.get("byteOffset", 0): bin0 + v.get("byteOffset", 0) + v["byteLength"]] for v in views]


def decode_with_host(hostlib, blob: bytes):
    raw = np.frombuffer(blob, np.uint8)
    w, h = C.c_uint32(), C.c_uint32()
    out = np.zeros(64 * 64 * 4, np.uint8)
    assert hostlib.rth_decode_image(abi.u8ptr(raw), raw.size, C.byref(w), C.byref(h), abi.u8ptr(out), out.size) == 0, hostlib.rth_last_error()
    return out[: w.value * h.value * 4].reshape(h.value, w.value, 4).copy()


def load_cpp(hostlib, data: bytes, tmp_path, name="file"):
    from test_host_cpp import CppScene
    path = Path(tmp_path) / f"{name}.glb"
    path.write_bytes(data)
    return CppScene(hostlib, path)


def cpp_error(hostlib, data: bytes, tmp_path) -> str:
    path = Path(tmp_path) / "refused.glb"
    path.write_bytes(data)
    h = C.c_void_p()
    rc = hostlib.rth_load_glb(str(path).encode(), C.byref(h))
    if rc == 0:
        hostlib.rth_scene_free(h)
        return ""
    return hostlib.rth_last_error().decode()


# ----------------------------------------------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------------------------------------------
def _reference_tree():
    """the directory oracle/Makefile builds the reference's files from: $REF, or the recipe's own default"""
    m = re.search(r"^REF \?= *(\S+)", (REPO / "oracle" / "Makefile").read_text(), re.M)
    return Path(os.environ.get("REF") or m.group(1))


def test_the_reference_library_is_built_where_the_reference_is_at_hand():
    """with the reference's sources present, running against the stored vectors only would hide that `make -C oracle ref` is broken"""
    tree = _reference_tree()
    if (tree / "deps" / "tiny_gltf.cpp").exists():
        assert REF.exists(), "the reference's glTF parser is at hand but oracle/_ref/libref_gltf.so is not built: make -C oracle ref"
    assert REF.exists() or STORED.exists()


def test_the_crafted_files_stay_small(files):
    for name, data in files.items():
        assert len(data) < 64 * 1024, name
        if name in REFUSED:
            continue
        jlen = struct.unpack_from("<I", data, 12)[0]
        for a in json.loads(data[20:20 + jlen].decode().replace("NaN", "0"))["accessors"]:
            assert a["count"] <= 900, name  # a few hundred vertices (index lists up to three per triangle)


@pytest.mark.parametrize("name", list(GOOD))
def test_reference_loads_the_file_cleanly(reference, files, tmp_path, name):
    """ret = true, no error, no warning-less surprises: and none of the reads the reference's source makes is undefined (the wrapper flags those)"""
    ref = reference.load(files[name], tmp_path, keep_images=name in RENDERED)
    assert int(ref["ret"][0]) == 1 and text_of(ref, "err") == "", text_of(ref, "err")
    assert text_of(ref, "ub") == "", text_of(ref, "ub")
    assert text_of(ref, "warn") == ""


def _compare_scene(exp: Expected, got, what: str, materials, camera):
    """`got`: positions, normals, uvs, indices, tri_instance; materials = per instance (transform, normal_mat, rt_material bytes); camera = (pos, dir, focal)"""
    for f in ("positions", "normals", "uvs"):
        np.testing.assert_array_equal(bits(getattr(got, f)), bits(getattr(exp, f)), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(got.indices, exp.indices, err_msg=f"{what}: indices")
    np.testing.assert_array_equal(got.tri_instance, exp.tri_instance, err_msg=f"{what}: triangle-to-instance")
    assert len(materials) == len(exp.transforms), f"{what}: instance count"
    for i, (xf, nm, rec) in enumerate(materials):
        np.testing.assert_array_equal(bits(xf), bits(exp.transforms[i]), err_msg=f"{what}: transform of instance {i}")
        np.testing.assert_array_equal(bits(nm), bits(exp.normal_mats[i]), err_msg=f"{what}: normal matrix of instance {i}")
        want = exp.material_record(exp.inst_gltf_material[i])
        assert rec == want, f"{what}: material of instance {i} (glTF material {exp.inst_gltf_material[i]}): {abi_material(rec)} != {abi_material(want)}"
    pos, dr, focal = camera
    np.testing.assert_array_equal(bits(pos), bits(exp.camera[0]), err_msg=f"{what}: camera position")
    np.testing.assert_array_equal(bits(dr), bits(exp.camera[1]), err_msg=f"{what}: camera direction")
    np.testing.assert_array_equal(bits(focal), bits(exp.camera[2]), err_msg=f"{what}: focal length")


def abi_material(rec: bytes):
    m = abi.rt_material.from_buffer_copy(rec)
    return (m.type, m.tex_kind, tuple(m.color), m.tex_layer, tuple(m.emissive), m.roughness, m.ior)


@pytest.mark.parametrize("name", list(GOOD))
def test_cpp_loader_equals_the_references_parser(reference, hostlib, files, tmp_path, name):
    """rth_load_glb's rt_scene_desc, field by field and bit by bit, against the scene that follows from the reference's own parse"""
    exp = Expected(reference.load(files[name], tmp_path, keep_images=name in RENDERED))
    cs = load_cpp(hostlib, files[name], tmp_path, name)
    insts = [(np.array(list(i.transform), f32), np.array(list(i.normal_mat), f32), bytes(cs.materials[i.material])) for i in cs.instances]
    assert cs.has_camera
    _compare_scene(exp, cs, "C++ loader", insts, (cs.camera.position, cs.camera.direction, cs.camera.focal_length))
    np.testing.assert_array_equal(bits(list(cs.c.sky)), bits(exp.sky), err_msg="sky")
    assert cs.c.n_layers == exp.n_images  # layer i is image i: a material's tex_layer is the reference's image index (material_record)
    for i, blob in enumerate(embedded_images(files[name])):  # and each image decodes to the bytes tinygltf hands over
        img = decode_with_host(hostlib, blob)
        assert img.shape == (int(exp.ref[f"image.{i}.height"][0]), int(exp.ref[f"image.{i}.width"][0]), 4)
        assert hashlib.sha256(img.tobytes()).digest() == exp.ref[f"image.{i}.sha256"].tobytes(), f"image {i}"
        if name in RENDERED:
            np.testing.assert_array_equal(img, reference_images(exp.ref)[i])


@pytest.mark.parametrize("name", list(GOOD))
def test_python_loader_equals_the_references_parser(reference, files, tmp_path, name):
    """rtamd.scenes.load_glb (it decodes no textures: everything but the layers)"""
    exp = Expected(reference.load(files[name], tmp_path, keep_images=name in RENDERED))
    path = tmp_path / f"{name}.glb"
    path.write_bytes(files[name])
    sd = scenes.load_glb(path)
    c = sd.to_c()
    insts = [(sd.transforms[i], sd.normal_mats[i], bytes(c.materials[int(sd.inst_material[i])])) for i in range(sd.transforms.shape[0])]
    _compare_scene(exp, sd, "Python loader", insts, (sd.camera.position, sd.camera.direction, sd.camera.focal_length))
    np.testing.assert_array_equal(bits(sd.sky), bits(exp.sky), err_msg="sky")


def test_the_good_files_do_what_they_are_there_for(reference, files, tmp_path):
    """guards on the fixtures themselves: a file that stopped exercising its case would pass everything above for nothing"""
    ref = {name: reference.load(files[name], tmp_path, keep_images=name in RENDERED) for name in GOOD}
    cls = lambda name: [int(ref[name][f"material.{i}.class"][0]) for i in range(int(ref[name]["n_materials"][0]))]
    assert cls("metallic_threshold") == [1, 1, 1, 0, 1, 0]  # 0.01 and both its double neighbours exceed (double)0.01f; 0.01f itself does not
    assert cls("ior_transmission") == [0, 0, 2, 2, 2] and [float(ref["ior_transmission"][f"material.{i}.ior"][0]) for i in (2, 3, 4)] == [float(f32(1.7)), 2.0, 0.0]
    assert cls("material_defaults") == [1, 1, 1, 1] and float(ref["material_defaults"]["material.0.roughness"][0]) == 1.0
    e = ref["emissive"]
    assert [e[f"material.{i}.emissive"].tolist() for i in (0, 3)] == [[0, 0, 0]] * 2 and e["material.1.emissive"].tolist() == [3.0, 1.5, 0.75]
    t = ref["texture_permutations"]
    assert [int(t[f"material.{i}.image"][0]) for i in range(4)] == [0, 1, 2, -1]  # index -> source: 1 -> 0, 2 -> 1, 0 -> 2
    assert int(ref["two_scenes_scene_1"]["scene"][0]) == 1 and int(ref["two_scenes_scene_absent"]["scene"][0]) == 0 and int(ref["two_scenes_scene_absent"]["default_scene"][0]) == -1
    assert int(ref["cameras"]["camera_node_index"][0]) == 2 and ref["cameras"]["camera_yfov"][0] == f32(0.305)
    assert f32(1.0 / np.tan(0.305 / 2.0)) != f32(f32(1.0) / _tanf(f32(f32(0.305) / f32(2.0))))  # the yfov tells the float formula from the double one
    n = ref["numbers"]
    assert bits(n["node.0.translation"].astype(f32)).tolist() == bits([100.0, 0.001, 0.0]).tolist()  # "-0" is the INTEGER 0 in the reference's JSON library: +0
    assert bits(n["node.1.translation"].astype(f32)).tolist() == bits([-0.0, 0.1, 1.0]).tolist() and n["node.1.scale"].tolist() == [16777217.0, 12345678901234567890.0, 1e-3]
    assert n["node.2.translation"].tolist() == [5e-324, 0.0, 16777217.0] and f32(n["node.2.translation"][2]) == f32(16777216.0)
    assert bits(n["material.1.base_color"]).tolist() == bits([0.0, -0.0, -0.0]).tolist() and bits(n["material.1.emissive"]).tolist() == bits([0.0, -0.0, 0.0]).tolist()
    assert "sky_color" not in ref["sky_wrong_length"] and "sky_strength" in ref["sky_wrong_length"] and "sky_color" not in ref["sky_not_numbers"]
    assert ref["sky_integer_spellings"]["sky_color"].tolist() == [1.0, 0.0, 2.0] and ref["sky_integer_spellings"]["sky_strength"].tolist() == [3.0]
    h = ref["hierarchy"]
    assert h["visit_order"].tolist() == [0, 1, 2, 3, 4, 5] and h["node.1.matrix"].size == 16 and h["node.1.translation"].size == 0 and h["node.2.translation"].size == 0
    assert h["mesh_primitives"].tolist() == [3, 1]


@pytest.mark.parametrize("name", list(UNDEFINED))
def test_stated_deviations_where_the_reference_is_undefined(reference, hostlib, files, tmp_path, name):
    """The closed list of DESIGN §2: tinygltf takes the file, and the reference's source then reads what is not there (the wrapper names the
    read). The loaders do what the table says: an error with this text, or the documented default."""
    _, flag, error = UNDEFINED[name]
    ref = reference.load(files[name], tmp_path)
    assert int(ref["ret"][0]) == 1 and text_of(ref, "err") == ""
    if flag is not None:
        assert flag in text_of(ref, "ub"), text_of(ref, "ub")
    got = cpp_error(hostlib, files[name], tmp_path)
    path = tmp_path / f"{name}.glb"
    path.write_bytes(files[name])
    if error is not None:
        assert got == error
        with pytest.raises((KeyError, ValueError)):
            scenes.load_glb(path)
        return
    assert got == ""
    cs, sd = load_cpp(hostlib, files[name], tmp_path, name), scenes.load_glb(path)
    if name == "no_material":  # the glTF default material (tiny_gltf.h's Material defaults): base colour 1, metallic 1 -> METALLIC, roughness 1
        for rec in (bytes(cs.materials[cs.instances[0].material]), bytes(sd.to_c().materials[int(sd.inst_material[0])])):
            assert abi_material(rec) == (abi.RT_MAT_METALLIC, abi.RT_TEX_COLOR, (1.0, 1.0, 1.0), 0, (0.0, 0.0, 0.0), 1.0, 1.5)
    elif name == "png_16_bit":  # decoded to RGBA8 by the high byte of every sample, as stb_image's 8-bit entry point does (tests/test_ref_stb.py)
        assert int(ref["image.0.bits"][0]) == 16 and cs.c.n_layers == 1
        np.testing.assert_array_equal(decode_with_host(hostlib, embedded_images(files[name])[0]), _picture(9, 6, 10, 4))
    elif name == "camera_on_node_0":  # `if (camera_node_index)` is false for 0 (src/scene.cpp:109): the reference renders from uninitialised members;
        assert int(ref["camera_node_index"][0]) == 0 and "camera_yfov" not in ref  # the loaders take the node's camera like any other
        assert cs.has_camera and tuple(cs.camera.position) == (1.0, 2.0, 3.0) and tuple(sd.camera.position) == (1.0, 2.0, 3.0)
    elif name == "no_camera":  # the documented default pose: the eye at the origin, looking down -z, focal length 1
        assert not cs.has_camera
        for cam in (cs.camera, sd.camera):
            assert (tuple(cam.position), tuple(cam.direction), cam.focal_length) == ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 1.0)


@pytest.mark.parametrize("name", list(REFUSED))
def test_files_tinygltf_refuses_are_refused(reference, hostlib, files, tmp_path, name):
    """where the reference's parser refuses a file (ret = false, the reference throws: src/scene.cpp:68-70), both loaders refuse it too"""
    ref_text, cpp_text = REFUSED[name]
    ref = reference.load(files[name], tmp_path)
    assert int(ref["ret"][0]) == 0 and ref_text in text_of(ref, "err"), text_of(ref, "err")
    assert cpp_text in cpp_error(hostlib, files[name], tmp_path)
    path = tmp_path / f"{name}.glb"
    path.write_bytes(files[name])
    with pytest.raises(ValueError):
        scenes.load_glb(path)

"""Generates tests/golden/ref_gltf/ref_gltf.npz: what the reference's own glTF parser returns for every file tests/test_ref_gltf.py
crafts, so that those tests (and the GPU check of tests/test_gpu_cli.py) also run where the reference's parser cannot be built.

It needs oracle/_ref/libref_gltf.so (`make -C oracle ref`, where the reference's sources are at hand) and the product's host library
(build()). It runs tests/test_ref_gltf.py against the live library and keeps every named array the wrapper (oracle/ref_gltf.cpp)
returned, under the SHA-256 of the file: the small fields whole, decoded images as SHA-256 digests (whole as well for the two files
the GPU check renders). Run from the repo root:  python tests/golden/make_ref_gltf.py
"""
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent.parent
OUT = Path(__file__).resolve().parent / "ref_gltf" / "ref_gltf.npz"


def main() -> int:
    env = dict(os.environ, RT_REF_GLTF_RECORD=str(OUT))
    return subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", str(REPO / "tests" / "test_ref_gltf.py")], cwd=REPO, env=env)


if __name__ == "__main__":
    sys.exit(main())

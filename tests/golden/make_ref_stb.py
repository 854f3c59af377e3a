"""Generates tests/golden/ref_stb/ref_stb.npz: what the reference's own stb_image / stb_image_resize2 return for every input of
tests/test_ref_stb.py, so that those tests also run where the reference's decoder cannot be built.

It needs oracle/_ref/libref_stb.so (`make -C oracle ref`, where the reference's sources are at hand) and the product's host
library (build()). It runs tests/test_ref_stb.py against the live library and keeps every result: decoded images as SHA-256
digests, baked layers as a digest plus a fixed sample of texels (test_ref_stb.LAYER_TEXELS), each under the SHA-256 of its
input. Run from the repo root:  python tests/golden/make_ref_stb.py
"""
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent.parent
OUT = Path(__file__).resolve().parent / "ref_stb" / "ref_stb.npz"  # (its own directory: tests/golden/*.npz are the render fixtures)


def main() -> int:
    env = dict(os.environ, RT_REF_STB_RECORD=str(OUT))
    return subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", str(REPO / "tests" / "test_ref_stb.py")], cwd=REPO, env=env)


if __name__ == "__main__":
    sys.exit(main())

"""Developer probe: the bounded wait of the sliced kernels (RT_INJECT_SLICE_LOSS / RT_SLICE_WAIT_CAP, developer build). Each case in a child process
with a time limit, so that a kernel that does not end is killed and reported instead of hanging the call.
   usage: slice_loss_probe.py            (parent)    |    slice_loss_probe.py child <mega|wave> <inject 0|1> <cap> <slices>"""
import os
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))

if len(sys.argv) > 1 and sys.argv[1] == "child":
    which, inject, cap, slices = sys.argv[2], sys.argv[3] == "1", sys.argv[4], int(sys.argv[5])
    from rtamd import abi, scenes
    from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer
    lib = abi.load_developer_library()
    sd = scenes.get_scene("cornell"); sc = Scene(sd, 0, lib=lib); cam = Camera.for_scene(sd, (96, 64))
    r = (MegakernelRenderer if which == "mega" else WavefrontRenderer)(sc, (96, 64), 6, 6)
    r.set_schedule(pixel_slices=slices)
    ref = r.render_frame(cam)
    print(f"  plain frame: {ref.device_ms:.2f} ms, {ref.pixel_slices} slices", flush=True)
    if inject:
        os.environ["RT_INJECT_SLICE_LOSS"] = "1"
    if cap != "-":
        os.environ["RT_SLICE_WAIT_CAP"] = cap
    t0 = time.perf_counter()
    try:
        fr = r.render_frame(cam)
        print(f"  frame returned in {time.perf_counter() - t0:.2f} s: {fr.device_ms:.2f} ms device, rays {fr.rays} (plain {ref.rays})", flush=True)
    except abi.RtError as e:
        print(f"  error after {time.perf_counter() - t0:.2f} s: {e}", flush=True)
    sys.exit(0)

for case in [tuple(c.split(",")) for c in (sys.argv[1:] or ["mega,0,3000,2", "mega,1,3000,2"])]:
    print("case", *case, flush=True)
    try:
        p = subprocess.run([sys.executable, "-u", __file__, "child", *case], timeout=90, capture_output=True, text=True)
        print(p.stdout, p.stderr[-400:] if p.returncode else "", flush=True)
    except subprocess.TimeoutExpired as e:
        print("  KILLED after 90 s:", (e.stdout or b"").decode()[-300:] if isinstance(e.stdout, bytes) else e.stdout, flush=True)
        break  # a kernel that did not end: no further GPU step in this call

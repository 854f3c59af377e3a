"""The wave loop's tunables, one library per call (RT_MI355X_LIB): the bench frame and the voxel terrain at 1080p, 64 spp, depth 10, both one-launch
renderers; median and minimum device ms of 5 frames after one warm-up, with the frame's digest and ray count (every variant renders the same frame).
The compile-time tunables are one developer library each (scripts/build_variant.sh NAME -DRT_DEVELOPER_KNOBS plus -DRT_VOTE_INNER=2 -DRT_VOTE_LEAF=3,
-DRT_MEGA_SHADE_PCT=70, -DRT_MEGA_UNROLL=4, -DRT_FINISH_UNROLL=4); the slice bounds are RT_MEGA_SLICE_BOUNDS of any developer library. Run the
unchanged library between the variants: its spread is the yardstick (profiles/wave_loop_sweep.txt).
usage: RT_MI355X_LIB=<library> wave_loop_sweep.py NAME [slice bounds of the megakernel on the atrium, cases separated by ';', e.g. "auto;44,60;off"]"""
import hashlib, os, statistics, sys
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import scenes
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer
name = sys.argv[1]
cases = sys.argv[2].split(";") if len(sys.argv) > 2 else ["auto"]
W, H, SPP, DEPTH = 1920, 1080, 64, 10
for sname, sd in (("atrium", scenes.atrium_scene(4)), ("voxel", scenes.voxel_scene(4))):
    sc = Scene(sd, 0); cam = Camera.for_scene(sd, (W, H))
    for cls in (MegakernelRenderer, WavefrontRenderer):
        for case in (cases if (cls is MegakernelRenderer and sname == "atrium") else ["auto"]):
            os.environ.pop("RT_MEGA_SLICE_BOUNDS", None)
            if case != "auto": os.environ["RT_MEGA_SLICE_BOUNDS"] = case
            r = cls(sc, (W, H), DEPTH, SPP)
            fr = r.render_frame(cam, want_f32=True, want_u8=False)
            digest = hashlib.sha1(fr.rgba_f32.tobytes()).hexdigest()[:10]
            ms = [r.render_frame(cam, want_f32=False, want_u8=False).device_ms for _ in range(5)]
            med = statistics.median(ms)
            print(f"{name:10s} {sname:7s} {cls.__name__[:-8]:10s} slices {case:>12s} -> {fr.pixel_slices}  median {med:8.3f} ms  min {min(ms):8.3f}  {fr.rays / med / 1e3:8.1f} Mrays/s  rays {fr.rays} frame {digest}", flush=True)
            r.close()
    sc.close()

import os, sys, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pytracer_amd import abi, flatten, scenes, _lib
from pytracer_amd.device import DeviceScene
W, H = 1280, 720
S = int(sys.argv[1]) if len(sys.argv) > 1 else 0
flat = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
cam = flatten.flatten_camera(scenes.synthetic_camera(W, H))
par = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=S, out_format=abi.OUT_F32)
ds = DeviceScene(flat)
for _ in range(3):
    out = ds.render(cam, par)
q = (C.c_ulonglong * 16)()
_lib.lib().pt_debug_read_queue(ds._h, q)
t = np.array([q[i] for i in range(1, 9)], dtype=np.float64)
names = ["coords", "cone", "cull+LDS", "sample setup+primary ray", "tile query", "shade+accum", "store", "loop top"]
nw = ((ds.stats().grid + 63) // 64) * 4  # sampled workgroups only
if ds.stats().kernel == abi.KERNEL_TILE4:  # 16x16 tiles, one per wave; every 16th workgroup reports
    names = ["prologue", "cone", "cull", "dome tile", "four rays", "query", "shade", "store"]
    nw = ((ds.stats().grid + 15) // 16) * 4
# a -DPT_DEBUG_HEAVY=<cycles> build sums the waves above that many cycles only, of every 4th workgroup: give the same number as the
# second argument and the sums are divided by the number of THOSE waves (from the per-wave log of the same frame)
HEAVY = int(sys.argv[2]) if len(sys.argv) > 2 else 0
if HEAVY and ds.stats().kernel == abi.KERNEL_TILE4:
    n = ds.stats().grid * 4
    buf = (C.c_ulonglong * (8 * n))()
    _lib.lib().pt_debug_read_unitlog(buf, n)
    tot = np.frombuffer(buf, dtype=np.uint64).reshape(n, 8)[:, 0]
    nw = max(1, int(((((np.arange(n) // 4) & 3) == 0) & (tot > HEAVY)).sum()))
    print(f"waves above {HEAVY} cycles among those of every 4th workgroup: {nw}")
print("kernel ms", ds.stats().kernel_ms, "sampled waves", nw, "tiles/wave", 14400 / (ds.stats().grid * 4))
for n, v in zip(names, t):
    print(f"{n:26s} {v / nw:10.0f} cycles/wave  {100 * v / t.sum():5.1f} %")
print("sum per wave", t.sum() / nw)
if ds.stats().kernel == abi.KERNEL_TILE4:  # (its own figure since section 5 ends in front of it; not part of the sum above)
    # the wave's wait for its own palette loads; in builds from before the palette, the wait at the workgroup barrier
    print(f"{'wait in front of shading':26s} {q[9] / nw:10.0f} cycles/wave")
if ds.stats().kernel == abi.KERNEL_TILE4:
    print(f"longest wave {q[12]} cycles; waves above 16 / 24 / 32 kcycles: {q[13]} / {q[14]} / {q[15]} of the {nw} sampled")

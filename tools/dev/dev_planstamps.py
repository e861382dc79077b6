"""Step clocks of fx_planfused_kernel on config 2 (one 20-Msample stream; needs a -DFX_STAMPS build, see dev_walkstamps.py):
FXRX_LIB=gr-liquiddsp_amd/csrc/libfxrx_stamps.so python tools/dev/dev_planstamps.py"""
import importlib, sys, os, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
fx = importlib.import_module("gr-liquiddsp_amd")
import torch
xb, fb = fx.synth_stream(20_000_000, stream_id=0)
xd = torch.from_numpy(xb).cuda()
ctx = fx.RxContext(1)
for it in range(5):
    gf = ctx.process([xd]); ctx.reset()
    out = (C.c_uint32 * 8)()
    fx.lib().fxrx_debug_chain_stamps(ctx.h, C.byref(out))
    s = [out[1], out[2], out[6], out[7]]
    print("pass %d, %d frames: sizes/scan/counts %d, jobs and records %d, items and padding %d, fence %d cycles (shares %s)" % (
        it, len(gf), s[0], s[1], s[2], s[3], " ".join("%.0f%%" % (100.0 * v / max(1, sum(s))) for v in s)))

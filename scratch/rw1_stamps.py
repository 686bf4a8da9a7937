"""Cycle stamps of the resident-weights 3x3 kernel (64 -> 64 and 64 -> 32 at 240x320), three products on fp32 tensors and one product
on f16 / fp32 tensors, in both consumer loops (EGNE_RW_SHADOW=0: hand-over form, default: shadow form): per wave, cycles between
barriers (work) and at barriers (wait), per job; for the consumers the part of the work outside the tap loops (hand-over form: the
hand-over of a finished tile; shadow form: the last tile's flush).  MFMA issue per job is 16 cycles x 72 (one product) or 216 (three).
usage: python scratch/rw1_stamps.py [B]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import egne_amd
from egne_amd import _lib, engine
from egne_amd.engine import ConvLayer, Piece, Plan, SplitScale
DEV = torch.device('cuda:0')
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
L = _lib.lib()
L.egne_rw_debug.restype = C.c_int; L.egne_rw_debug.argtypes = [C.c_int, C.c_void_p]
CASES = (("3 products 64->64", 64, 64, 240, 320, False, 3), ("3 products 64->32", 64, 32, 240, 320, False, 3),
         ("conv1_2 f16", 64, 64, 240, 320, True, 1), ("conv1_2 fp32", 64, 64, 240, 320, False, 1), ("ms1 conv f16 in", 64, 32, 240, 320, True, 1))
for name, Cin, Cout, H, W, f16io, products in CASES:
    pl = Plan(DEV)
    if products == 1:
        pl.f16_products = 1
    w = torch.nn.Parameter(torch.randn(Cout, Cin, 3, 3, device=DEV) / (3 * Cin ** 0.5)); b = torch.nn.Parameter(torch.randn(Cout, device=DEV))
    layer = ConvLayer([w], [b], [(Cin, Cin)], pad=(1, 1), act=1); layer.split = True
    if f16io:
        xb = pl.buf16(B, H, W, Cin); xb.copy_((torch.randn(B, H, W, Cin, device=DEV).relu() * 64).half())
        pin = Piece(xb, 0, Cin); pin.f16s = SplitScale(); pin.f16s.value, pin.f16s.vmax = 64.0, 5.0
        ob = pl.buf16(B, H, W, Cout); pout = Piece(ob, 0, Cout); pout.f16s = SplitScale()
    else:
        xb = pl.buf(B, H, W, Cin); xb.normal_().relu_(); pin = Piece(xb, 0, Cin)
        ob = pl.buf(B, H, W, Cout); pout = Piece(ob, 0, Cout)
    pl.conv(layer, [pin], pout, B, H, W)
    assert pl.meta[0][0] == "conv_f16x3:rw", pl.meta
    for form in ("0", "1"):
        os.environ["EGNE_RW_SHADOW"] = form
        for _ in range(3): pl.run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10): pl.run()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        L.egne_rw_debug(64, None)
        e0.record(); pl.run(); e1.record(); torch.cuda.synchronize()
        ms_st = e0.elapsed_time(e1)
        buf = np.zeros(256 * 8 * 4, dtype=np.uint64)
        L.egne_rw_debug(0, buf.ctypes.data_as(C.c_void_p))
        st = buf.reshape(256, 8, 4).astype(np.float64)
        jobs = np.maximum(st[:, :, 2], 1)
        prod, cons = st[:, :4], st[:, 4:]
        print("%-18s %s B=%d  %.3f ms (stamped %.3f);  jobs per workgroup %.0f;  per job: producers work %.0f wait %.0f | consumers work %.0f (of it outside the tap loops %.0f) wait %.0f   (100 MHz stamps)" % (
            name, "shadow   " if form == "1" else "hand-over", B, ms, ms_st, st[:, :, 2].mean(), (prod[:, :, 0] / jobs[:, :4]).mean(), (prod[:, :, 1] / jobs[:, :4]).mean(),
            (cons[:, :, 0] / jobs[:, 4:]).mean(), (cons[:, :, 3] / jobs[:, 4:]).mean(), (cons[:, :, 1] / jobs[:, 4:]).mean()), flush=True)

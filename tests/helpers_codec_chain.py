"""Shared by the GPU codec tests: the decode spelled out as the unfused chain of older C-ABI calls -- gi2d_quant_decompress
per attribute, gi2d_fast_project_bin, gi2d_fast_rasterize_forward (the fitting forward), then a clamp in torch -- for the
whole picture (unfused_chain) and for a codec.View (unfused_view_chain).  None of it goes through the codec's own kernels:
it is what the fused decode and the draw kernel are held against, bit for bit."""
import ctypes as C

import numpy as np
import torch

from oracle import codec_oracle as CO

DEV = "cuda:0"


def unfused_chain(blob):
    """gi2d_quant_decompress per attribute -> gi2d_fast_project_bin -> gi2d_fast_rasterize_forward, fed from the
    stream through the numpy oracle's unpack."""
    from gaussianimage_plus_amd import _lib
    from gaussianimage_plus_amd.quantize import LOG, LSQ, make_spec
    h = CO.parse(blob)
    kind, n, bits, side = h["kind"], h["num_points"], h["bits"], h["side"]
    codes = torch.from_numpy(CO.unpack(kind, bits, n, h["payload"]).astype(np.float32)).to(DEV)
    groups = [(0, 2), (2, 5), (5, 8)] if kind == 1 else [(0, 2), (2, 4), (4, 5), (5, 8)]
    st = torch.cuda.current_stream().cuda_stream
    vals = []
    for lo, hi in groups:
        kinds = [LOG if (kind == 1 and k in (2, 4)) else LSQ for k in range(lo, hi)]
        spec = make_spec(kinds, [0] * (hi - lo), [1] * (hi - lo))
        params = torch.zeros(hi - lo, 4, device=DEV)
        params[:, 0:2] = torch.from_numpy(side[lo:hi]).to(DEV)
        c = codes[:, lo:hi].contiguous()
        out = torch.empty_like(c)
        _lib.call("gi2d_quant_decompress", C.byref(spec), n, c.data_ptr(), params.data_ptr(), out.data_ptr(), st)
        vals.append(out)
    W, H = h["width"], h["height"]
    tx, ty = (W + 15) // 16, (H + 15) // 16
    f = lambda *s: torch.empty(s, device=DEV)
    i = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)
    xys, depths, radii, conics, nth = f(n, 2), f(n), i(n), f(n, 3), i(n)
    ws = torch.empty(_lib.load().gi2d_fast_workspace_bytes(n, tx, ty), dtype=torch.uint8, device=DEV)
    status, img, opac, bg = torch.zeros(4, dtype=torch.int32, device=DEV), f(H, W, 3), torch.ones(n, device=DEV), torch.ones(3, device=DEV)
    _lib.call("gi2d_fast_workspace_init", ws.data_ptr(), ws.numel(), n, tx, ty, st)
    p1 = vals[2].data_ptr() if kind == 2 else None
    _lib.call("gi2d_fast_project_bin", kind, n, h["clip_coe"], vals[0].data_ptr(), vals[1].data_ptr(), p1,
              vals[-1].data_ptr(), opac.data_ptr(), H, W, tx, ty, h["radius_clip"], xys.data_ptr(), depths.data_ptr(),
              radii.data_ptr(), conics.data_ptr(), nth.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(), st)
    _lib.call("gi2d_fast_rasterize_forward", n, tx, ty, W, H, bg.data_ptr(), ws.data_ptr(), ws.numel(),
              status.data_ptr(), None, None, img.data_ptr(), st)
    assert status[1].item() == 0
    return dict(xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, colors=vals[-1], image=img.clamp(0, 1),
                values=torch.cat(vals, 1))


def dequantised(blob):
    """The dequantised values [N, 8] on the device, as test_codec_gpu.py::unfused_chain makes them: gi2d_quant_decompress
    per attribute, fed from the stream through the numpy oracle's unpack."""
    from gaussianimage_plus_amd import _lib
    from gaussianimage_plus_amd.quantize import LOG, LSQ, make_spec
    h = CO.parse(blob)
    kind, n, bits, side = h["kind"], h["num_points"], h["bits"], h["side"]
    codes = torch.from_numpy(CO.unpack(kind, bits, n, h["payload"]).astype(np.float32)).to(DEV)
    groups = [(0, 2), (2, 5), (5, 8)] if kind == 1 else [(0, 2), (2, 4), (4, 5), (5, 8)]
    st = torch.cuda.current_stream().cuda_stream
    vals = []
    for lo, hi in groups:
        kinds = [LOG if (kind == 1 and k in (2, 4)) else LSQ for k in range(lo, hi)]
        spec = make_spec(kinds, [0] * (hi - lo), [1] * (hi - lo))
        params = torch.zeros(hi - lo, 4, device=DEV)
        params[:, 0:2] = torch.from_numpy(side[lo:hi]).to(DEV)
        c = codes[:, lo:hi].contiguous()
        out = torch.empty_like(c)
        _lib.call("gi2d_quant_decompress", C.byref(spec), n, c.data_ptr(), params.data_ptr(), out.data_ptr(), st)
        vals.append(out)
    return torch.cat(vals, 1)


def unfused_view_chain(blob, view):
    """view_parameters with torch on the device -> gi2d_fast_project_bin -> gi2d_fast_rasterize_forward at the view's
    size with the scaled radius_clip."""
    from gaussianimage_plus_amd import _lib, codec
    h = CO.parse(blob)
    kind, n = h["kind"], h["num_points"]
    t = codec.view_parameters(kind, dequantised(blob), view)
    xy, col = t[:, 0:2].contiguous(), t[:, 5:8].contiguous()
    p0 = t[:, 2:5].contiguous() if kind == 1 else t[:, 2:4].contiguous()
    p1 = t[:, 4:5].contiguous() if kind == 2 else None
    W, H = view.width, view.height
    rc = float(np.float32(h["radius_clip"]) * np.float32(view.scale))
    tx, ty = (W + 15) // 16, (H + 15) // 16
    f = lambda *s: torch.empty(s, device=DEV)
    i = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)
    xys, depths, radii, conics, nth = f(n, 2), f(n), i(n), f(n, 3), i(n)
    ws = torch.empty(_lib.load().gi2d_fast_workspace_bytes(n, tx, ty), dtype=torch.uint8, device=DEV)
    status, img, opac, bg = torch.zeros(4, dtype=torch.int32, device=DEV), f(H, W, 3), torch.ones(n, device=DEV), torch.ones(3, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("gi2d_fast_workspace_init", ws.data_ptr(), ws.numel(), n, tx, ty, st)
    _lib.call("gi2d_fast_project_bin", kind, n, h["clip_coe"], xy.data_ptr(), p0.data_ptr(),
              p1.data_ptr() if p1 is not None else None, col.data_ptr(), opac.data_ptr(), H, W, tx, ty, rc, xys.data_ptr(),
              depths.data_ptr(), radii.data_ptr(), conics.data_ptr(), nth.data_ptr(), ws.data_ptr(), ws.numel(),
              status.data_ptr(), st)
    _lib.call("gi2d_fast_rasterize_forward", n, tx, ty, W, H, bg.data_ptr(), ws.data_ptr(), ws.numel(),
              status.data_ptr(), None, None, img.data_ptr(), st)
    assert status[1].item() == 0
    return dict(xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, colors=col, image=img.clamp(0, 1))

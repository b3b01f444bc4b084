"""Development aid: the whole state of a few quantisation-aware fits with fixed seeds, as one .npz -- to be written by two
builds of the library (GI2D_LIB=<path> picks another one) and compared word for word:
    quant_state_dump.py dump <covariance | scale_rot> <out.npz>
    quant_state_dump.py compare <a.npz> <b.npz>      (one line per array: shape, differing 32-bit words; exit 1 if any)
Runs: single image 96x144, N = 3000 (warm-up 20, debug gradients, calls of 1 + 3 + 5 quantised iterations); single image
512x768, N = 30000 and N = 40000 (50 quantised iterations: parked entries; 64- and 256-lane workgroups); two tiny batches
through BatchFitter whose populations sit on the wave and workgroup edges."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

STATE_ROWS = ("xyz", "chol", "feat", "m_xyz", "v_xyz", "m_chol", "v_chol", "m_feat", "v_feat")
QROWS = ("qparams", "qm", "qv", "best_qparams", "qfeat")
OUTPUTS = ("out_img", "tile_sse", "best_xyz", "best_chol", "best_feat", "best_bound", "best_sse", "best_info")
TINY = ([(17, 33, 63), (32, 48, 64), (48, 32, 65)], [(40, 40, 257), (16, 16, 2)])


def state_of(fit, tag, out):
    names = STATE_ROWS + QROWS + OUTPUTS + ("dbg_grads", "dbg_qgrads") + (("qrange",) if fit.kind == "covariance" else ())
    for nm in names:
        t = getattr(fit, nm, None)
        if t is None:
            continue
        if t.dim() and t.shape[0] in (fit.n, fit.cap) and nm not in ("out_img", "tile_sse"):
            t = t[:fit.n]
        out[f"{tag}/{nm}"] = t.detach().cpu().numpy()


def dump(kind, path):
    import torch
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import BatchFitter, NativeFitter
    from gaussianimage_plus_amd import _lib
    print("library:", _lib.LIB_PATH, _lib.version())
    lr = 0.018 if kind == "covariance" else 1e-3
    out = {}

    def fitter(h, w, n, seed, warm, debug):
        f = NativeFitter(synthetic_image(h, w, seed).to("cuda:0"), n, kind=kind, lr=lr, eps=1e-15, seed=seed,
                         track_best=True, debug_grads=debug)
        f.train(warm)
        f.enable_quantize(12, None, 6, debug_grads=debug)
        return f

    f = fitter(96, 144, 3000, 5, 20, True)
    for c in (1, 3, 5):
        f.train(c)
    state_of(f, "small", out)
    # per-gaussian kernels in 64-lane workgroups up to N = 32768, in 256-lane ones above
    for tag, n in (("large", 30000), ("large256", 40000)):
        f = fitter(512, 768, n, 6, 20, False)
        f.train(50)
        f.check_status()
        state_of(f, tag, out)
    for b, sizes in enumerate(TINY):
        fs = [fitter(h, w, n, 20 + 8 * b + i, 40, False) for i, (h, w, n) in enumerate(sizes)]
        batch = BatchFitter(fs)
        for c in (1, 3, 5):
            batch.train(c)
        for i, f in enumerate(fs):
            state_of(f, f"batch{b}.{i}", out)
    torch.cuda.synchronize()
    for f in fs:
        f.check_status()
    np.savez(path, **out)
    print(f"{kind}: {len(out)} arrays -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    total = 0
    for nm in a.files:
        x, y = a[nm], b[nm]
        assert x.shape == y.shape and x.dtype == y.dtype and x.dtype.itemsize == 4, nm
        diff = int((x.view(np.uint32) != y.view(np.uint32)).sum())  # raw words: NaNs compare too
        total += diff
        print(f"{nm:28s} {str(x.shape):16s} differing words {diff}")
    print(f"{len(a.files)} arrays, {total} differing words")
    return total


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)

"""GPU tests (-m gpu): nnmk_joint_count / nnmk_joint_write on buffers at odd element offsets between guard bands (tests/embed.py).
x, y, both lengths, offsets and out each start an odd number of elements into a byte buffer filled with one value, and the
workspace has exactly nnmk_joint_workspace_bytes bytes between its guards, aligned to 8 and not to 256; after the calls the inputs
hold their bits, every guard holds its fill byte, and offsets and the first min(N, cap) rows equal tools/joint_model.py bit for bit
(the rows past them still hold the fill byte)."""
import numpy as np
import pytest

import embed
import joint_cases as JC

pytestmark = pytest.mark.gpu

DT_CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
CASES = [c for c in JC.cases() if c["name"] in ("t63-b3-d5-5-w3", "t65-b3-d64-65-w0", "t131-b70-d1-w2", "mix-float32-float64-float32",
                                                "live-w3", "cap-below", "cap-above", "all-dropped")]


@pytest.mark.parametrize("offsets", [(1, 3, 5, 7, 1, 3), (3, 1, 1, 1, 5, 1)], ids=["1-3-5-7-1-3", "3-1-1-1-5-1"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_offset_buffers_between_guard_bands(case, offsets):
    import torch
    from nnmnkwii_amd import _joint_hip as JH
    L = JH.lib()
    dx, dy, do = (np.dtype(t) for t in case["dtypes"])
    X, Y = JC.typed(case)
    B, Tmax, Dx = X.shape
    Dy = 0 if Y is None else Y.shape[2]
    W, cap = JC.width(case), JC.capacity(case)
    ox, oy, olx, oly, oo, oout = offsets
    x, y = embed.embedded(X, ox), embed.embedded(Y, oy)
    lx, ly = embed.embedded(case["len_x"], olx), embed.embedded(case["len_y"] if Y is not None else None, oly)
    offs = embed.Embedded((B + 1,), np.int64, oo)
    out = embed.Embedded((cap, W), do, oout)
    need = L.nnmk_joint_workspace_bytes(B, Tmax)
    ws = embed.Workspace(need, align=8)
    assert x.ptr() % 16 and ws.ptr() % 256 == 8 and x.ptr() % dx.itemsize == 0
    nw, wl, wu, wc = JH.pack_windows(case["wins"])
    src = (DT_CODE[dx], x.ptr(), Dx, embed.ptr(lx), Dx, DT_CODE[dy], embed.ptr(y), Dy, embed.ptr(ly), Dy, B, Tmax, nw, wl.ctypes.data, wu.ctypes.data,
           wc.ctypes.data)
    dev = torch.device("cuda", torch.cuda.current_device())
    n0 = L.nnmk_joint_launch_count()
    rc = L.nnmk_joint_count(dev.index, None, *src, case["keep"], case["eps"], DT_CODE[do], ws.ptr(), need, offs.ptr())
    assert rc == 0, L.mlpg_hip_last_error()
    rc = L.nnmk_joint_write(dev.index, None, *src, ws.ptr(), need, DT_CODE[do], out.ptr() if cap else None, W, cap)
    assert rc == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    assert L.nnmk_joint_launch_count() == n0 + 1 + (cap > 0)
    assert embed.failed(inputs=dict(x=x, y=y, len_x=lx, len_y=ly), outputs=dict(offsets=offs, out=out), workspaces=dict(workspace=ws)) == []
    rows, want_offs = JC.expected(case)
    n = min(len(rows), cap)
    assert JC.same_bits(offs.host(), want_offs) and JC.same_bits(out.host()[:n], rows[:n])
    assert bool((out.bytes_view()[n * W * do.itemsize:] == out.fill).all().item())

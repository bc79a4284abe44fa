"""GPU tests (-m gpu) of the waveform kernels (csrc/wave_codec.hip).  The device result equals tools/wave_model.py
bit for bit (integer views, so NaNs and -0.0 count) wherever no device transcendental is involved -- pre-emphasis, the table,
every de-emphasis with its tiles, segments and warm-up -- on the case list of tests/wave_cases.py through the C entries; the float
mu-law stays within its documented bound of the numpy evaluation.  The classes of the whole 16-bit grid equal the reference's at
every point, at each of a thread's four sample positions, for mu 255 and 256 and both dtypes.  The fused chains are held against
the reference's recorded results; a row of a wider tensor, the six functions with numpy, tensors and scalars, one launch per
call."""
import os

import numpy as np
import pytest
import torch

import wave_cases as WC
from wave_cases import WM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = WC.cases()


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "wave_ref.npz"))


def launches():
    from nnmnkwii_amd import _wave_hip
    return _wave_hip.lib().nnmk_wave_launch_count()


def device_run(case):
    """tests/test_wave_host_cpu.py's host_run on the device: (rc, x after the call, y after it)."""
    from nnmnkwii_amd import HipExtensionError, _wave_hip as WH
    x0, y0 = WC.buffers(case)
    Lmax = case["X"].shape[1]
    ld_x, off_x, ld_y, off_y = WC.layout_of(case)
    xt, yt = torch.from_numpy(x0).cuda(), torch.from_numpy(y0).cuda()
    lengths = None if case["lengths"] is None else torch.from_numpy(case["lengths"]).cuda()
    xs = xt[:, off_x:off_x + Lmax]
    if case["mode"] in ("inplace", "refused"):
        ys = xs.view(yt.dtype) if xs.element_size() == yt.element_size() else torch.empty(0)
    else:
        ys = yt[:, off_y:off_y + Lmax]
    rc = 0
    try:
        if case["mode"] == "refused" and ys.numel() == 0:
            # unequal element sizes: no tensor view says "the same pointer", so the C entry is called as the host test calls it
            L = WH.lib()
            rc = L.nnmk_wave_encode(0, None, WH._code(xs), xs.data_ptr(), ld_x, None, xs.shape[0], Lmax, case["coef"] is not None, 0.0,
                                    case["stage"], case["mu"], WM.CODE[y0.dtype], xs.data_ptr(), ld_x)
        elif case["op"] == "encode":
            WH.encode(xs, lengths, case["coef"], case["stage"], case["mu"], ys)
        else:
            table = torch.from_numpy(WM.inv_mulaw_table(case["mu"])).cuda() if case["stage"] == WM.QUANTIZE else None
            WH.decode(xs, lengths, case["stage"], case["mu"], table, case["coef"], min(case["segment"], 1 << 40), ys)
    except HipExtensionError as e:
        assert "(-1): wave:" in str(e), e
        rc = -1
    return rc, xt.cpu().numpy(), yt.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_list_through_the_c_entries(case):
    n0 = launches()
    got = device_run(case)
    assert launches() == n0 + (case["mode"] != "refused")
    assert WC.verdict(case, got) == []
    if case["mode"] != "refused":
        again = device_run(case)
        assert WC.same_bits(got[1], again[1]) and WC.same_bits(got[2], again[2])


@pytest.mark.parametrize("mu", [256, 255])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_classes_on_the_whole_16_bit_grid_in_one_launch(G, mu, dt):
    """(4, 65536): row r is the grid rotated by r samples, so every point meets each of a thread's four sample positions."""
    from nnmnkwii_amd import preprocessing as P
    k = np.arange(-32768, 32768)
    X = np.stack([np.roll(k, r) for r in range(4)]) / 32768.0
    want = np.stack([np.roll(G["q_%d_%s" % (mu, ("f32", "f64")[dt == np.float64])], r) for r in range(4)])
    n0 = launches()
    got = P.wave_encode_batch(torch.from_numpy(X.astype(dt)).cuda(), mu=mu, dtype=torch.int16)
    assert launches() == n0 + 1
    got = got.cpu().numpy()
    assert got.dtype == np.int16 and np.array_equal(got, want), "%d points differ" % (got != want).sum()
    row = got[0]
    assert row[0] == 0 and row[32768] == mu // 2 and want[0][65535] == mu - 1                  # x = -1, 0, and the last point below +1
    marks = np.array([-1.0, 1.0, 0.0, -0.0], dtype=dt)
    assert P.mulaw_quantize(marks, mu).tolist() == [0, mu, mu // 2, mu // 2]
    assert P.mulaw_quantize(torch.from_numpy(marks).cuda(), mu).tolist() == [0, mu, mu // 2, mu // 2]
    assert P.mulaw_quantize(1.0, mu) == mu and P.mulaw_quantize(-1.0, mu) == 0 and isinstance(P.mulaw_quantize(0.0, mu), int)


def test_decode_table_is_the_literal_expression_of_the_numpy_at_hand(G):
    from nnmnkwii_amd import preprocessing as P
    for mu in (255, 256, 1023, 4999):
        y = np.arange(mu + 1).astype(np.float32)
        y = 2 * y / mu - 1
        literal = np.sign(y) * (1.0 / mu) * ((1.0 + mu) ** np.abs(y) - 1.0)               # generic.py:171-172 and :104
        assert literal.dtype == np.float32
        n0 = launches()
        got = P.inv_mulaw_quantize(np.arange(mu + 1), mu)
        assert launches() == n0 + 1
        assert WC.same_bits(got, literal) and WC.same_bits(got, G["table_%d" % mu])
        gt = P.inv_mulaw_quantize(torch.arange(mu + 1, device="cuda", dtype=torch.int32).reshape(-1, 1), mu)
        assert gt.is_cuda and gt.shape == (mu + 1, 1) and WC.same_bits(gt.cpu().numpy().ravel(), literal)
    assert WC.same_bits(P.inv_mulaw_quantize(np.array([[-4, 0], [300, 256]]), 256), G["table_256"][[[0, 0], [256, 256]]])
    assert WC.same_bits(P.inv_mulaw_quantize(np.uint8(128), 255), G["table_255"][128])


def test_fused_chains_against_the_reference(G):
    from nnmnkwii_amd import preprocessing as P
    X, classes, wave = G["chain_x"], G["chain_classes"], G["chain_wave"]
    Xt = torch.from_numpy(X).cuda()
    n0 = launches()
    got = P.wave_encode_batch(Xt, None, 0.97, 256, dtype=torch.int16)
    assert launches() == n0 + 1
    got = got.cpu().numpy()
    v = WM.mulaw_v(np.stack([WM.preemphasis(x, 0.97) for x in X]), 256)
    band = np.abs(v - np.rint(v)) <= 2.0 ** -15
    differ = got != classes
    print("pre-emphasis -> quantise, float32, on the device: %d of %d classes differ from the reference's float32 path; share of "
          "samples within 2^-15 bins of an edge %.2e (allowed 2e-4)" % (differ.sum(), differ.size, band.mean()))
    assert (band | ~differ).all() and band.mean() <= 2e-4
    assert np.array_equal(got, WM.encode_batch(X, None, 0.97, WM.QUANTIZE, 256, np.int16))
    for dt in (torch.uint8, torch.int32, torch.int64):
        alt = P.wave_encode_batch(Xt, None, 0.97, 255 if dt == torch.uint8 else 256, dtype=dt)
        assert alt.dtype == dt and np.array_equal(alt.cpu().numpy(), WM.encode_batch(X, None, 0.97, WM.QUANTIZE, 255 if dt == torch.uint8 else 256))
    # classes -> table -> de-emphasis in one launch: the model's bits, and the reference's values within the two bounds
    c32 = float(np.float32(0.97))
    for segment in (None, 2048):
        n0 = launches()
        dec = P.wave_decode_batch(torch.from_numpy(classes).cuda(), None, 256, 0.97, segment=segment)
        assert launches() == n0 + 1
        dec = dec.cpu().numpy()
        assert WC.same_bits(dec, WM.decode_batch(classes, None, WM.QUANTIZE, 256, c32, 0 if segment is None else segment, np.float32))
        worst = 0.0
        for b in range(len(classes)):
            y64, e_kernel = WM.scan(WM.front(classes[b], WM.QUANTIZE, 256), c32, None, 0 if segment is None else segment)
            bound = WM.ref_bound(wave[b], 0.97) + e_kernel + 2.0 ** -24 * np.abs(y64)
            err = np.abs(dec[b].astype(np.float64) - wave[b])
            assert (err <= bound).all()
            worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
        print("classes -> table -> de-emphasis on the device (segment %s): largest error / bound %.3f" % (segment, worst))
    # companded floats there and back, each within its bound of the numpy evaluation
    m = P.wave_encode_batch(Xt, quantize=False).cpu().numpy()
    exact = WM._mulaw64(X.astype(np.float64), 256)
    err = np.abs(m.astype(np.float64) - exact)
    assert m.dtype == np.float32 and (err <= (WM.MULAW_ULPS * 2.0 ** -53 + 2.0 ** -24) * np.abs(exact)).all()
    m64 = torch.from_numpy(exact).cuda()
    back = P.wave_decode_batch(m64).cpu().numpy()
    want = WM._inv_mulaw64(exact, 256)
    tol = WM.INV_MULAW_ULPS * 2.0 ** -53 * 257.0 ** np.abs(exact) / 256
    print("float inv_mulaw on the device: largest error / bound %.3f; mulaw: %.3f"
          % ((np.abs(back - want) / tol).max(), (np.abs(P.wave_encode_batch(torch.from_numpy(X.astype(np.float64)).cuda(), quantize=False).cpu().numpy()
                                                        - exact) / np.maximum(WM.MULAW_ULPS * 2.0 ** -53 * np.abs(exact), 1e-300)).max()))
    assert back.dtype == np.float64 and (np.abs(back - want) <= tol).all()


def test_a_row_of_a_wider_tensor_and_in_place():
    from nnmnkwii_amd import preprocessing as P
    rng = np.random.RandomState(8)
    B, Lmax, wide = 3, 2500, 2500 + 37
    lengths = np.array([2500, 1025, 0])
    X = np.stack([WC.wave(rng, wide) for _ in range(B)]).astype(np.float32)
    Xt = torch.from_numpy(X).cuda()
    rows = Xt[:, 11:11 + Lmax]                                                       # utterance stride 2537 > Lmax, nothing aligned
    out = torch.full((B, wide), 249, dtype=torch.uint8, device="cuda")
    n0 = launches()
    got = P.wave_encode_batch(rows, lengths, 0.97, 255, out=out[:, 5:5 + Lmax])
    assert launches() == n0 + 1 and got.data_ptr() == out[:, 5:].data_ptr()
    want = WM.encode_batch(X[:, 11:11 + Lmax], lengths, 0.97, WM.QUANTIZE, 255, np.uint8)
    res = out.cpu().numpy()
    assert np.array_equal(res[:, 5:5 + Lmax], want) and (res[:, :5] == 249).all() and (res[:, 5 + Lmax:] == 249).all()
    assert WC.same_bits(Xt.cpu().numpy(), X)
    # in place without emphasis: companded floats over the waveform
    got = P.wave_encode_batch(rows, lengths, None, 256, quantize=False, out=rows)
    assert got.data_ptr() == rows.data_ptr()
    res = Xt.cpu().numpy()
    exact = WM.encode_batch(X[:, 11:11 + Lmax], lengths, None, WM.MULAW, 256, np.float64)
    assert (np.abs(res[:, 11:11 + Lmax] - exact) <= (WM.MULAW_ULPS * 2.0 ** -53 + 2.0 ** -24) * np.abs(exact)).all()
    assert WC.same_bits(res[:, :11], X[:, :11]) and WC.same_bits(res[:, 11 + Lmax:], X[:, 11 + Lmax:])
    # decode into a row slice, lengths as a device tensor, float64 out of classes
    dst = torch.full((B, wide), -7.0, dtype=torch.float64, device="cuda")
    P.wave_decode_batch(out[:, 5:5 + Lmax], torch.from_numpy(lengths).cuda(), 255, 0.85, out=dst[:, 1:1 + Lmax], segment=1024)
    want = WM.decode_batch(want, lengths, WM.QUANTIZE, 255, float(np.float32(0.85)), 1024, np.float64)
    res = dst.cpu().numpy()
    assert WC.same_bits(np.ascontiguousarray(res[:, 1:1 + Lmax]), want) and (res[:, 0] == -7).all() and (res[:, 1 + Lmax:] == -7).all()


def test_the_six_functions_with_numpy_tensors_and_scalars(G):
    from nnmnkwii_amd import preprocessing as P
    for i in (20, 25, int(G["n"]) - 2, int(G["n"]) - 1):                             # float32 and float64 tracks, the longest ones among them
        x, c, pre, inv = G["x%d" % i], float(G["coef"][i]), G["pre%d" % i], G["inv%d" % i]
        x0 = x.copy()
        n0 = launches()
        y = P.preemphasis(x, c)
        assert launches() == n0 + 1
        assert isinstance(y, np.ndarray) and WC.same_bits(y, pre) and WC.same_bits(x, x0)
        yt = P.preemphasis(torch.from_numpy(x).cuda(), c)
        assert yt.is_cuda and yt.shape == x.shape and WC.same_bits(yt.cpu().numpy(), pre)
        z = P.inv_preemphasis(x, c)
        cd = float(x.dtype.type(c))
        assert z.dtype == x.dtype and WC.same_bits(z, WM.decode(x, WM.PLAIN, coef=cd, segment=0, dtype=x.dtype))
        bound = WM.ref_bound(inv, c) + WM.scan(x.astype(np.float64), cd, None, 0)[1] + WM.U[x.dtype] * np.abs(inv.astype(np.float64))
        assert (np.abs(z.astype(np.float64) - inv) <= bound).all()
        zt = P.inv_preemphasis(torch.from_numpy(x).cuda(), c)
        assert zt.is_cuda and WC.same_bits(zt.cpu().numpy(), z)
        rt = P.inv_preemphasis(P.preemphasis(x, c), c)
        assert np.allclose(rt, x, rtol=0, atol=(2e-5 if x.dtype == np.float32 else 1e-12) / (1 - abs(c)))
    x = (np.arange(-50, 51) / 50.0).reshape(101, 1)
    for dt in (np.float32, np.float64):
        m = P.mulaw(x.astype(dt), 255)
        assert m.dtype == dt and m.shape == x.shape and np.allclose(m, WM.mulaw(x.astype(dt), 255), rtol=4e-7 if dt == np.float32 else 4e-15, atol=0)
        r = P.inv_mulaw(m, 255)
        assert r.dtype == dt and np.allclose(r, x, rtol=0, atol=4e-6 if dt == np.float32 else 1e-14)
        q = P.mulaw_quantize(x.astype(dt), 255)
        assert q.dtype == np.int64 and q.shape == x.shape and np.array_equal(q, WM.mulaw_quantize(x.astype(dt), 255))
        qt = P.mulaw_quantize(torch.from_numpy(x.astype(dt)).cuda(), 255)
        assert qt.is_cuda and qt.dtype == torch.int64 and np.array_equal(qt.cpu().numpy(), q)
        assert WC.same_bits(P.inv_mulaw_quantize(q, 255), WM.inv_mulaw_quantize(q, 255))
    assert isinstance(P.mulaw(0.5), np.float64) and abs(P.mulaw(0.5) - WM.mulaw(np.array(0.5))) < 1e-15 and P.mulaw(np.arange(3)).dtype == np.float64
    assert P.mulaw(np.zeros(0)).shape == (0,) and P.preemphasis(np.zeros(0, dtype=np.float32)).shape == (0,)
    cpu = P.preemphasis(torch.from_numpy(G["x20"]), 0.97)
    assert torch.is_tensor(cpu) and not cpu.is_cuda and WC.same_bits(cpu.numpy(), G["pre20"])

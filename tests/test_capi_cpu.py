"""CPU-side checks (-m "not gpu"): the C-ABI library loads and exports every
symbol include/mlpg_hip.h declares, argument validation works without a GPU,
and the host-side mirrors of the reference helpers behave like the reference."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cases import WINDOW_SETS
from oracle import mlpg as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def test_exports_match_header(L):
    from nnmnkwii_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    declared = set(re.findall(r"\b(mlpg_hip_\w+)\s*\(", hdr))
    assert declared == set(_hip.EXPORTS)
    for name in declared:
        assert getattr(L, name) is not None
    assert L.mlpg_hip_abi_version() == _hip.ABI_VERSION == 14


def test_argument_validation_without_gpu(L):
    wl = np.array([0, 1], dtype=np.int32)
    wu = np.array([0, 1], dtype=np.int32)
    wc = np.array([1.0, -0.5, 0.0, 0.5])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fake = ctypes.c_void_p(64)
    # D not a multiple of num_windows
    rc = L.mlpg_hip_forward(0, None, 1, 0, fake, fake, 0, None, 1, 4, 5, 2, p(wl), p(wu), p(wc), fake, None)
    assert rc == -1 and b"multiple" in L.mlpg_hip_last_error()
    # bad dtype
    rc = L.mlpg_hip_forward(0, None, 7, 0, fake, fake, 0, None, 1, 4, 4, 2, p(wl), p(wu), p(wc), fake, None)
    assert rc == -1
    # window extent too large
    wl2 = np.array([0, 9], dtype=np.int32)
    rc = L.mlpg_hip_forward(0, None, 1, 0, fake, fake, 0, None, 1, 4, 4, 2, p(wl2), p(wu), p(wc), fake, None)
    assert rc == -1 and b"extents" in L.mlpg_hip_last_error()
    # empty batch is a no-op
    rc = L.mlpg_hip_forward(0, None, 1, 0, None, fake, 0, None, 0, 4, 4, 2, p(wl), p(wu), p(wc), None, None)
    assert rc == 0
    # multi-stream entry: a stream that does not fit the row, and an empty table
    from nnmnkwii_amd._hip import StreamDesc
    tab = (StreamDesc * 1)(StreamDesc(4, 0, 1, 2, 0))
    rc = L.mlpg_hip_forward_streams(0, None, 1, 0, fake, fake, 0, 5, None, 1, 4, 1, ctypes.addressof(tab), 2,
                                    p(wl), p(wu), p(wc), fake, 1, None)
    assert rc == -1 and b"does not fit" in L.mlpg_hip_last_error()
    rc = L.mlpg_hip_forward_streams(0, None, 1, 0, fake, fake, 0, 5, None, 1, 4, 0, None, 0, None, None, None, fake, 1, None)
    assert rc == 0
    # modulation spectrum: DFT length >= 2 and >= T
    rc = L.mlpg_hip_modspec(0, None, fake, 1, 1, 2, 1, 0, fake, None)
    assert rc == -1 and b"at least 2" in L.mlpg_hip_last_error()
    rc = L.mlpg_hip_modspec_smoothing(0, None, fake, 1, 100, 2, 64, 0, 10, 1, fake)
    assert rc == -1 and b"time length" in L.mlpg_hip_last_error()
    rc = L.mlpg_hip_fastdtw_l2(0, None, fake, fake, fake, fake, 1, 4, 4, 2, 0, fake, fake, fake, fake)
    assert rc == -1
    assert L.mlpg_hip_device_count() >= 0


def test_device_out_of_range_is_refused_before_the_runtime_is_touched(L):
    """Every device-pointer solve entry point answers a device outside [0, 16) with MLPG_HIP_EINVAL naming it (the pointers
    are fakes: a call that got as far as a launch would fault)."""
    from nnmnkwii_amd._hip import StreamDesc
    wl = np.array([0, 1], dtype=np.int32)
    wu = np.array([0, 1], dtype=np.int32)
    wc = np.array([1.0, -0.5, 0.0, 0.5])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fake = ctypes.c_void_p(64)
    win = (p(wl), p(wu), p(wc))
    tab = (StreamDesc * 1)(StreamDesc(0, 0, 2, 2, 0))
    for dev in (-1, 16, 99):
        calls = [
            L.mlpg_hip_forward(dev, None, 1, 0, fake, fake, 0, None, 1, 4, 4, 2, *win, fake, None),
            L.mlpg_hip_backward(dev, None, 1, 1, 0, fake, 0, fake, None, 1, 4, 4, 2, *win, fake, None),
            L.mlpg_hip_forward_streams(dev, None, 1, 0, fake, fake, 0, 4, None, 1, 4, 1, ctypes.addressof(tab), 2, *win, fake, 2, None),
            L.mlpg_hip_unit_mse_form(dev, None, 0, 0, 2, 100, 4, 2, *win),
            L.mlpg_hip_unit_mse_step(dev, None, 0, fake, fake, None, 2, 100, 4, 2, *win, 1.0, None, fake, fake, None, fake, 1 << 20),
        ]
        for k, rc in enumerate(calls):
            assert rc == -1, (dev, k, rc)
        # (each call's text, asked right behind it)
        assert L.mlpg_hip_forward(dev, None, 1, 0, fake, fake, 0, None, 1, 4, 4, 2, *win, fake, None) == -1
        assert b"forward: bad device" in L.mlpg_hip_last_error()
        assert L.mlpg_hip_forward_streams(dev, None, 1, 0, fake, fake, 0, 4, None, 1, 4, 1, ctypes.addressof(tab), 2, *win, fake, 2,
                                          None) == -1
        assert b"forward_streams: bad device" in L.mlpg_hip_last_error()


def test_forward_streams_refuses_a_forced_family_before_any_launch(L):
    """A forced family one stream cannot take is answered from the plan, with no device in sight: the stream and the family
    are named and no counter moves (mlpg_hip_backward_streams' guarantee, tests/test_backward_streams_capi_cpu.py)."""
    from nnmnkwii_amd._hip import StreamDesc
    wl = np.array([0, 1, 1, 2], dtype=np.int32)
    wu = np.array([0, 1, 1, 2], dtype=np.int32)
    wc = np.array([1.0, -0.5, 0.0, 0.5, 1.0, -2.0, 1.0, 1.0, -8.0, 0.0, 8.0, -1.0])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fake = ctypes.c_void_p(64)
    tab = (StreamDesc * 2)(StreamDesc(0, 0, 4, 3, 0), StreamDesc(12, 4, 2, 1, 3))      # std windows | one window of extent 2

    def call(algo, var_mode=0, Tmax=8, n=2):
        c0 = [L.mlpg_hip_launch_count(k) for k in range(16)]
        rc = L.mlpg_hip_forward_streams(0, None, 1, algo, fake, fake, var_mode, 14, None, 2, Tmax, n, ctypes.addressof(tab), 4,
                                        p(wl), p(wu), p(wc), fake, 6, None)
        assert [L.mlpg_hip_launch_count(k) for k in range(16)] == c0
        return rc, L.mlpg_hip_last_error().decode()

    for kw, word in [(dict(algo=3), "stream 1: MLPG_HIP_ALGO_STRIP"),                 # extent 2
                     (dict(algo=2), "stream 1: MLPG_HIP_ALGO_WAVE"),
                     (dict(algo=2, Tmax=4000, n=1), "stream 0: MLPG_HIP_ALGO_WAVE"),  # beyond 2048 frames
                     (dict(algo=5), "stream 0: MLPG_HIP_ALGO_CONST"),                 # per-frame variances
                     (dict(algo=7), "stream 0: MLPG_HIP_ALGO_FIR"),
                     (dict(algo=9), "algo")]:
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, rc, err)


def test_forward_streams_refuses_the_windowed_families_beyond_the_2_gb_window(L):
    """rows_fit_buffer (csrc/common.h): Tmax * row stride * 8 < 2^31 - 1 for the kernels that address an utterance through a buffer
    descriptor.  130 * 2064888 * 8 = 2^31 - 128 is inside; with one element more per row -- on the input or on the output side,
    in either dtype -- a forced STRIP, CONST, CHUNK or FIR is refused from the plan, before a device is selected: EINVAL, the
    stream and the family named, no counter moved (the pointers are fakes: a call that got as far as a launch would fault).
    tests/test_far_rows_gpu.py runs the accepted side of the rule, and AUTO beyond it."""
    from nnmnkwii_amd._hip import StreamDesc
    wl = np.array([0, 1, 1, 2], dtype=np.int32)
    wu = np.array([0, 1, 1, 2], dtype=np.int32)
    wc = np.array([1.0, -0.5, 0.0, 0.5, 1.0, -2.0, 1.0, 1.0, -8.0, 0.0, 8.0, -1.0])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fake = ctypes.c_void_p(64)
    std = (StreamDesc * 1)(StreamDesc(0, 0, 40, 3, 0))                # the standard windows
    ext2 = (StreamDesc * 1)(StreamDesc(0, 0, 10, 1, 3))               # one window of extent 2
    assert 130 * 2064888 * 8 == 2 ** 31 - 128

    def call(tab, dtype, algo, var_mode, ld_in, ld_out):
        c0 = [L.mlpg_hip_launch_count(k) for k in range(16)]
        rc = L.mlpg_hip_forward_streams(0, None, dtype, algo, fake, fake, var_mode, ld_in, None, 3, 130, 1, ctypes.addressof(tab), 4,
                                        p(wl), p(wu), p(wc), fake, ld_out, None)
        assert [L.mlpg_hip_launch_count(k) for k in range(16)] == c0
        return rc, L.mlpg_hip_last_error().decode()

    for ld_in, ld_out in ((2064889, 40), (120, 2064889)):
        for dtype in (0, 1):
            for tab, algo, var_mode, name in ((std, 3, 0, "STRIP"), (std, 5, 1, "CONST"), (std, 5, 2, "CONST"), (ext2, 6, 0, "CHUNK"),
                                              (std, 7, 2, "FIR")):
                if name == "FIR" and dtype == 1:
                    continue                                          # (float64: refused whatever the stride)
                rc, err = call(tab, dtype, algo, var_mode, max(ld_in, 30) if tab is ext2 else ld_in, ld_out)
                assert rc == -1 and "stream 0: MLPG_HIP_ALGO_" + name in err, (ld_in, ld_out, dtype, name, rc, err)
    # a row stride the int32 columns of the table cannot address is refused as a size
    rc, err = call(std, 1, 0, 0, 2 ** 31, 40)
    assert rc == -1 and "oversized" in err, err


def test_unit_mse_form_validates_without_gpu(L):
    wl = np.array([0, 1], dtype=np.int32)
    wu = np.array([0, 1], dtype=np.int32)
    wc = np.array([1.0, -0.5, 0.0, 0.5])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L.mlpg_hip_unit_mse_form(0, None, 0, 0, 2, 100, 5, 2, p(wl), p(wu), p(wc)) == -1      # D not a multiple of nw
    assert b"multiple" in L.mlpg_hip_last_error()
    assert L.mlpg_hip_unit_mse_form(0, None, 9, 0, 2, 100, 4, 2, p(wl), p(wu), p(wc)) == -1      # bad dtype
    assert L.mlpg_hip_unit_mse_form(0, None, 0, 0, 0, 100, 4, 2, p(wl), p(wu), p(wc)) == 1       # an empty batch: the step answers it
    assert L.mlpg_hip_launch_count(10) >= 0 and L.mlpg_hip_launch_count(11) >= 0 and L.mlpg_hip_launch_count(12) == -1


def test_backward_host_validates_without_gpu(L):
    """mlpg_hip_backward_host (ABI 14: the literal paramgen.mlpg_grad call on host memory): argument errors and empty
    batches are answered before any device is touched."""
    wl = np.array([0, 1], dtype=np.int32)
    wu = np.array([0, 1], dtype=np.int32)
    wc = np.array([1.0, -0.5, 0.0, 0.5])
    go = np.zeros((1, 4, 2))
    var = np.ones((1, 4, 4))
    grad = np.zeros((1, 4, 4), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    args = (p(wl), p(wu), p(wc), p(grad), None)
    assert L.mlpg_hip_backward_host(0, 1, 0, 0, p(var), 0, p(go), None, 1, 4, 5, 2, *args) == -1       # D not a multiple of nw
    assert b"bad sizes" in L.mlpg_hip_last_error()
    assert L.mlpg_hip_backward_host(0, 7, 0, 0, p(var), 0, p(go), None, 1, 4, 4, 2, *args) == -1       # bad dtype
    assert L.mlpg_hip_backward_host(0, 1, 0, 0, None, 0, p(go), None, 1, 4, 4, 2, *args) == -1         # per-frame variances, NULL
    assert L.mlpg_hip_backward_host(-1, 1, 0, 0, p(var), 0, p(go), None, 1, 4, 4, 2, *args) == -1       # bad device
    assert L.mlpg_hip_backward_host(0, 1, 0, 0, p(var), 0, p(go), None, 0, 4, 4, 2, *args) == 0        # an empty batch
    assert L.mlpg_hip_backward_host(0, 1, 0, 0, p(var), 0, p(go), None, 1, 0, 4, 2, *args) == 0        # no frames


def test_host_copy_pool_copies_every_byte_and_survives_shutdown(L):
    """mlpg_hip_host_copy: the staging copy of the short host path (calling thread + helper threads, 64 KB slices claimed
    through one atomic word) -- sizes around the slice boundaries, back-to-back jobs (helpers awake), jobs behind a pause
    (helpers asleep), from two Python threads, and again after mlpg_hip_shutdown joined the helpers."""
    import threading
    import time
    rng = np.random.RandomState(0)
    src = rng.randint(0, 256, size=(9 << 20) + 13, dtype=np.uint8)

    def check(n, off=0):
        dst = np.full(n + 64, 0xA5, dtype=np.uint8)
        assert L.mlpg_hip_host_copy(dst.ctypes.data + 32, src.ctypes.data + off, n) == 0
        assert np.array_equal(dst[32:32 + n], src[off:off + n])
        assert (dst[:32] == 0xA5).all() and (dst[32 + n:] == 0xA5).all()       # nothing outside the range is touched

    for n in (0, 1, 65535, 65536, 65537, 131071, 131072, 131073, 1440000, 2880000, (9 << 20) + 13):
        check(n)
    for k in range(200):                         # back to back: the helpers are spinning
        check(int(rng.randint(1, 3 << 20)), int(rng.randint(0, 1 << 20)))
    for _ in range(3):                           # behind a pause: the helpers sleep and are woken
        time.sleep(0.01)
        check(1440000, 7)
    errs = []

    def run(seed):
        r = np.random.RandomState(seed)
        try:
            for _ in range(60):
                check(int(r.randint(1, 2 << 20)), int(r.randint(0, 1 << 20)))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(s,)) for s in (1, 2, 3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    L.mlpg_hip_shutdown()                        # joins the helpers; the next copy brings them up again
    check(2880000)
    L.mlpg_hip_shutdown()
    assert L.mlpg_hip_host_copy(None, None, 0) == 0 and L.mlpg_hip_host_copy(None, src.ctypes.data, 8) == -1


def test_cached_windows_follow_the_list():
    from nnmnkwii_amd import _hip
    w = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))]
    a = _hip.cached_windows(w)
    assert _hip.cached_windows(w) is a and a[3] == 2 and a[2].tolist() == [1.0, -0.5, 0.0, 0.5]
    w[1][2][0] = -0.25                                   # edited in place: packed afresh
    b = _hip.cached_windows(w)
    assert b is not a and b[2].tolist() == [1.0, -0.25, 0.0, 0.5]
    w.append((1, 1, np.array([1.0, -2.0, 1.0])))
    c = _hip.cached_windows(w)
    assert c[3] == 3 and _hip.cached_windows(w) is c
    assert _hip.cached_windows(c) is c                   # already packed
    wl = [(0, 0, [1.0]), (1, 0, (-1.0, 1.0))]            # plain sequences as coefficients
    d = _hip.cached_windows(wl)
    assert d[2].tolist() == [1.0, -1.0, 1.0] and _hip.cached_windows(wl) is d
    wl[1] = (1, 0, (-2.0, 2.0))
    assert _hip.cached_windows(wl)[2].tolist() == [1.0, -2.0, 2.0]
    with pytest.raises(AssertionError):
        _hip.cached_windows([(1, 1, np.array([1.0]))])


def test_current_device_index_survives_a_half_imported_torch(monkeypatch):
    """A numpy entry point called while another thread is inside `import torch` sees a module object without attributes in
    sys.modules (found by tools/dbg/lit_threads_soak.py): the device index falls back to 0 instead of raising."""
    import sys
    import types
    from nnmnkwii_amd import _hip
    monkeypatch.setitem(sys.modules, "torch", types.ModuleType("torch"))
    assert _hip.current_device_index() == 0
    assert _hip.current_device_index("cuda:3") == 3 and _hip.current_device_index(2) == 2


def test_pack_windows():
    from nnmnkwii_amd import _hip
    wl, wu, wc = _hip.pack_windows(WINDOW_SETS["wide3"])
    assert wl.tolist() == [0, 2, 2] and wu.tolist() == [0, 2, 2] and wc.shape == (11,)
    with pytest.raises(AssertionError):
        _hip.pack_windows([(1, 1, np.array([1.0]))])


def test_win_mats_and_full_window_mat():
    # reference: tests/test_paramgen.py:62-79
    from nnmnkwii_amd import paramgen as G
    for wname, windows in WINDOW_SETS.items():
        for T in (1, 2, 5, 10):
            win_mats = G.build_win_mats(windows, T)
            fulls = [w.full() for w in win_mats]
            for (l, u, c), w, f in zip(windows, win_mats, fulls):
                assert (w.l, w.u, w.transposed) == (l, u, True)
                assert np.array_equal(f, O.window_matrix(l, u, c, T))
                assert np.array_equal(w.T.full(), f.T)
            assert np.array_equal(G.full_window_mat(win_mats, T), np.vstack(fulls))


def test_reshape_means():
    # reference: tests/test_paramgen.py:98-110
    from nnmnkwii_amd import paramgen as G
    T, sd = 10, 2
    for windows in WINDOW_SETS.values():
        means = np.random.RandomState(0).rand(T, sd * len(windows))
        r = G.reshape_means(means, sd)
        assert r.shape == (T * len(windows), sd)
        assert G.reshape_means(r, sd) is r or len(windows) == 1
        assert np.array_equal(r, O.reshape_means(means, sd))


def test_no_cpu_fallback():
    """Without a GPU the product raises instead of silently computing on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nnmnkwii_amd import HipExtensionError
    from nnmnkwii_amd import paramgen as G
    with pytest.raises(HipExtensionError):
        G.mlpg(np.zeros((4, 3)), np.ones((4, 3)), WINDOW_SETS["std3"])


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "nnmnkwii_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), fn
                assert "liboracle" not in src, fn


def test_dtw_custom_dist_is_evaluated_on_the_host_and_needs_the_gpu_for_the_rest():
    from nnmnkwii_amd import HipExtensionError
    from nnmnkwii_amd.preprocessing.alignment import DTWAligner, _resolve_dist
    assert _resolve_dist(lambda x, y: 1.0 - float(x @ y)) is None
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    a = DTWAligner(dist=lambda x, y: 1.0 - float(x @ y))
    with pytest.raises(HipExtensionError):       # no CPU fallback for the DP either
        a.transform((np.ones((1, 3, 2)), np.ones((1, 3, 2))))
    d = DTWAligner()
    assert d.radius == 1 and d.verbose == 0 and callable(d.dist) and d.tie_rule == "first"


def test_dtw_broken_dist_warns_instead_of_falling_back_silently():
    """a `dist` that raises on the probe frames used to be swallowed (and the alignment silently went the
    per-cell host route); now it says so, once per process."""
    import warnings
    from nnmnkwii_amd.preprocessing import alignment as A
    A._warned.discard("probe")

    def broken(x, y):
        raise ValueError("typo")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert A._resolve_dist(broken) is None
        assert A._resolve_dist(broken) is None
    assert len([x for x in w if issubclass(x.category, RuntimeWarning) and "probe frames" in str(x.message)]) == 1


def test_compat_install_provides_the_reference_names():
    """nnmnkwii_amd.compat: user code written against ``nnmnkwii`` resolves to the HIP path (no GPU needed to import)."""
    import sys
    import nnmnkwii_amd.compat as compat
    from nnmnkwii_amd import paramgen as G
    from nnmnkwii_amd.preprocessing.alignment import DTWAligner
    assert "nnmnkwii" not in sys.modules
    compat.install()
    try:
        from nnmnkwii.paramgen import mlpg, unit_variance_mlpg_matrix   # noqa: F401
        from nnmnkwii.preprocessing.alignment import DTWAligner as D2, IterativeDTWAligner   # noqa: F401
        from nnmnkwii.baseline.gmm import MLPG   # noqa: F401
        from nnmnkwii.autograd import unit_variance_mlpg   # noqa: F401
        from nnmnkwii.util import apply_each2d_padded   # noqa: F401
        import nnmnkwii.preprocessing as P
        assert mlpg is G.mlpg and D2 is DTWAligner and P.modspec_smoothing is not None
        compat.install()          # idempotent
    finally:
        compat.uninstall()
    assert "nnmnkwii" not in sys.modules and "nnmnkwii.paramgen" not in sys.modules


def test_header_is_plain_c_and_a_c_program_links(tmp_path):
    """include/mlpg_hip.h is what a cgo / JNI / ctypes binding reads: it must compile as C (no C++-isms), and a C
    program must link against the library and get its ABI version -- no GPU needed for that."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    from nnmnkwii_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = _hip.SO_PATH
    if not os.path.exists(so):
        pytest.skip("library not built")
    src = tmp_path / "demo.c"
    src.write_text(
        '#include <stdio.h>\n#include "mlpg_hip.h"\n'
        "int main(void) {\n"
        "  mlpg_hip_stream_t s; s.in_col = 0; s.out_col = 0; s.static_dim = 1; s.num_windows = 0; s.win_first = 0; (void)s;\n"
        '  printf("%d %d %d\\n", mlpg_hip_abi_version(), MLPG_HIP_ALGO_CONST, MLPG_HIP_DIST_SCALED_SQL2_NP);\n'
        "  return 0;\n}\n")
    exe = tmp_path / "demo"
    cmd = [gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), str(src), "-o", str(exe), so,
           "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, env=env)
    assert out.returncode == 0, out.stdout
    assert out.stdout.split() == ["14", "5", "3"], out.stdout


def test_host_chunk_plan_deals_round_robin_and_covers_the_batch():
    """mlpg_hip_host_chunk_plan: the dealing logic of the host-memory entry points over a device list (pure host code).
    Chunks tile the batch in order without gaps; chunk c runs on list entry c % n, stream slot (c // n) % 2; at least
    four chunks per device when the batch allows; never an empty chunk."""
    from nnmnkwii_amd import _hip
    for n_items, target, ndev in [(256, 10, 1), (256, 10, 8), (37, 10, 1), (37, 1000, 3), (1, 5, 8), (1024, 90, 8), (5, 2, 4),
                                  (0, 4, 2)]:
        entry, slot, first, count = _hip.host_chunk_plan(n_items, target, ndev)
        assert count.sum() == n_items and (count > 0).all()
        assert (first == np.concatenate([[0], np.cumsum(count)[:-1]])).all()
        c = np.arange(len(entry))
        assert (entry == c % ndev).all() and (slot == (c // ndev) % 2).all()
        if len(count):
            assert count.max() <= target
            assert count[0] == max(1, min(target, -(-n_items // (4 * ndev))))      # about four chunks per device
            assert (count[:-1] == count[0]).all()
    # one device: exactly the two-slot alternation of the single-device call
    entry, slot, first, count = _hip.host_chunk_plan(37, 10, 1)
    assert entry.tolist() == [0, 0, 0, 0] and slot.tolist() == [0, 1, 0, 1] and count.tolist() == [10, 10, 10, 7]
    with pytest.raises(_hip.HipExtensionError):
        _hip.host_chunk_plan(10, 0, 1)
    assert _hip.device_list("all").size == 0 and _hip.device_list([1, 1, 0]).tolist() == [1, 1, 0]
    assert _hip.device_list(3).tolist() == [3] and _hip.device_list("cuda:2").tolist() == [2]


def test_one_hip_runtime_whichever_is_loaded_first():
    """Loading libmlpg_hip.so BEFORE torch must not bring a second HIP runtime into the process (the PyTorch-ROCm wheel ships its
    own copy; with two of them torch.cuda.is_available() turns False): checked in a fresh interpreter, library first."""
    code = r"""
import sys
sys.path.insert(0, %r)
from nnmnkwii_amd import _hip
_hip.lib()
import torch
libs = sorted(set(l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l))
print(len(libs), libs)
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert out.stdout.split()[0] == "1", out.stdout


def test_header_constants_match_the_python_binding():
    """Every MLPG_HIP_* integer constant of include/mlpg_hip.h that the ctypes binding mirrors has the same value there."""
    from nnmnkwii_amd import _hip
    src = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MLPG_HIP_([A-Z0-9_]+)\s+\(?(-?\d+)\)?", src, re.M)}
    pairs = {"ALGO_AUTO": _hip.ALGO_AUTO, "ALGO_GENERIC": _hip.ALGO_GENERIC, "ALGO_WAVE": _hip.ALGO_WAVE, "ALGO_STRIP": _hip.ALGO_STRIP,
             "ALGO_PIPE": _hip.ALGO_PIPE, "ALGO_CONST": _hip.ALGO_CONST, "ALGO_CHUNK": _hip.ALGO_CHUNK, "ALGO_FIR": _hip.ALGO_FIR,
             "F32": _hip.F32, "F64": _hip.F64, "VAR_FRAME": _hip.VAR_FRAME, "VAR_GLOBAL": _hip.VAR_GLOBAL, "VAR_UNIT": _hip.VAR_UNIT,
             "DIST_L2": _hip.DIST_L2, "DIST_SCALED_L2_NP": _hip.DIST_SCALED_L2_NP, "DIST_SCALED_L1_NP": _hip.DIST_SCALED_L1_NP,
             "DIST_SCALED_SQL2_NP": _hip.DIST_SCALED_SQL2_NP, "TIE_FIRST_MIN": _hip.TIE_FIRST_MIN, "TIE_DIAG_LAST": _hip.TIE_DIAG_LAST}
    for name, val in pairs.items():
        assert defs.get(name) == val, (name, defs.get(name), val)


def test_grids_beyond_the_thread_limit_are_refused_before_the_runtime_is_touched(L):
    """A grid is 32 bits of threads (workgroups * threads per workgroup < 2^32); a larger launch would run truncated and report
    nothing.  The entries that cannot cut their batch refuse it before a device is selected, the limit named.  For each: the call AT
    the bound passes the check (the refusal that comes next answers: a NULL pointer, a bad device, the second stream), one item more
    is refused.  Fake pointers throughout (a call that got as far as a launch would fault); no counter moves."""
    from nnmnkwii_amd._hip import StreamDesc
    fake = ctypes.c_void_p(64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    c0 = [L.mlpg_hip_launch_count(k) for k in range(44)]
    err = lambda: L.mlpg_hip_last_error().decode()  # noqa: E731
    most = ((1 << 24) - 1) * 256                                      # elements of a one-thread-per-element launch: 2^32 - 256
    wl, wu, wc = np.array([0], dtype=np.int32), np.array([0], dtype=np.int32), np.array([1.0])
    # mlpg_hip_delta_features: B * Tmax * D elements
    assert L.mlpg_hip_delta_features(0, None, 0, None, None, (1 << 24) - 1, 256, 1, 1, p(wl), p(wu), p(wc), None) == -1
    assert "NULL pointer" in err()
    assert L.mlpg_hip_delta_features(0, None, 0, None, None, 1 << 24, 256, 1, 1, p(wl), p(wu), p(wc), None) == -1
    assert "16777215 workgroups of 256 threads" in err()
    # mlpg_hip_gmm_convert: N * Dy elements
    assert L.mlpg_hip_gmm_convert(0, None, None, None, None, None, None, None, most // 256, 4, 256, 2, None) == -1 and "NULL pointer" in err()
    assert L.mlpg_hip_gmm_convert(0, None, None, None, None, None, None, None, most // 256 + 1, 4, 256, 2, None) == -1
    assert "16777215 workgroups of 256 threads" in err()
    # mlpg_hip_gather_path walks the utterances in slices: only ONE utterance of more than a grid is refused
    assert L.mlpg_hip_gather_path(0, None, 0, None, None, None, 1 << 30, 4, 4, 256, (1 << 24) - 1, None) == -1 and "NULL pointer" in err()
    assert L.mlpg_hip_gather_path(0, None, 0, None, None, None, 1, 4, 4, 256, 1 << 24, None) == -1
    assert "16777215 workgroups of 256 threads" in err()
    # the float64 modulation-spectrum entries walk the sequences in slices: no batch is refused for its size (the device is asked next)
    assert L.mlpg_hip_modspec(99, None, fake, (1 << 31) - 1, 2, 4, 2, 0, fake, None) == -1 and "bad device" in err()
    # a kernel family asked for by name, through the stream plan: stream 0 at its bound passes (stream 1 is refused for another
    # reason), one utterance more and stream 0 is refused for its grid.  FIR: 3 B + 1 workgroups of 512 threads at Tmax = 96;
    # CHUNK: 2 B workgroups of 64 threads in its reductions; GENERIC: B * sd * Tmax cells, one thread each.
    wl2 = np.array([0, 1, 2], dtype=np.int32)
    wc2 = np.array([1.0, -0.5, 0.0, 0.5, 1.0, -8.0, 0.0, 8.0, -1.0])
    static, delta, ext2 = (1, 0), (1, 1), (1, 2)                      # (num_windows, win_first)

    def streams(algo, dtype, var_mode, B, Tmax, s0, s1, sd1=1):
        tab = (StreamDesc * 2)(StreamDesc(0, 0, 1, *s0), StreamDesc(1, 1, sd1, *s1))
        rc = L.mlpg_hip_forward_streams(0, None, dtype, algo, fake, fake, var_mode, 1 + sd1, None, B, Tmax, 2, ctypes.addressof(tab), 3,
                                        p(wl2), p(wl2), p(wc2), fake, 1 + sd1, None)
        return rc, err()
    fir_most = ((1 << 23) - 2) // 3
    rc, e = streams(7, 0, 2, fir_most, 96, static, delta)
    assert rc == -1 and "stream 1: MLPG_HIP_ALGO_FIR" in e, e
    rc, e = streams(7, 0, 2, fir_most + 1, 96, static, delta)
    assert rc == -1 and "stream 0: MLPG_HIP_ALGO_FIR" in e and "8388607" in e, e
    rc, e = streams(6, 1, 0, (1 << 25) - 1, 8, ext2, static)
    assert rc == -1 and "stream 1: MLPG_HIP_ALGO_CHUNK" in e, e
    rc, e = streams(6, 1, 0, 1 << 25, 8, ext2, static)
    assert rc == -1 and "stream 0: MLPG_HIP_ALGO_CHUNK" in e and "67108863" in e, e
    rc, e = streams(1, 1, 0, (1 << 24) - 1, 256, static, static, sd1=2)
    assert rc == -1 and "stream 1: MLPG_HIP_ALGO_GENERIC" in e and "16777215" in e, e
    rc, e = streams(1, 1, 0, 1 << 24, 256, static, static, sd1=2)
    assert rc == -1 and "stream 0: MLPG_HIP_ALGO_GENERIC" in e and "16777215" in e, e
    # a pass-through stream is ONE launch of the copy, a thread per element: stream 0 (one column) at 2^32 - 256 elements passes
    # (stream 1 is refused for its family), one utterance more is refused for the copy's grid
    rc, e = streams(3, 1, 0, (1 << 24) - 1, 256, (0, 0), ext2)
    assert rc == -1 and "stream 1: MLPG_HIP_ALGO_STRIP" in e, e
    rc, e = streams(3, 1, 0, 1 << 24, 256, (0, 0), ext2)
    assert rc == -1 and "stream 0: " in e and "elements to copy" in e and "16777215 workgroups of 256 threads" in e, e
    assert [L.mlpg_hip_launch_count(k) for k in range(44)] == c0


def test_the_restated_plan_refuses_a_family_for_its_grid_where_the_library_does(L):
    """tests/stream_plan.py restates chunk_grid_fits, fir_grid_fits and generic_grid_fits (csrc/mlpg_chunk.hip, mlpg_fir.hip,
    mlpg_generic.hip).  A family by name, two streams, fake pointers: at the bound the library takes stream 0 and refuses stream 1
    (a window set or a width the family does not take), one utterance more and it refuses stream 0 -- and the plan predicts a
    launch of the family for stream 0 at the bound, and raises Refused with the family's name one over.  The bounds: FIR 3 B + 1 <=
    2^23 - 1 workgroups at Tmax = 96; CHUNK 2 B <= 2^26 - 1 in its reductions, and ceil(B K / 4) <= 2^24 - 1 in its passes (K = 13
    chunks of 20 frames at Tmax = 256: B = 5162220); GENERIC B * sd * Tmax <= 2^32 - 256 cells."""
    import stream_plan as SP
    from nnmnkwii_amd._hip import StreamDesc
    fake = ctypes.c_void_p(64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    c0 = [L.mlpg_hip_launch_count(k) for k in range(44)]
    wl = np.array([0, 1, 2], dtype=np.int32)
    wc = np.array([1.0, -0.5, 0.0, 0.5, 1.0, -8.0, 0.0, 8.0, -1.0])
    static, delta, ext2 = 0, 1, 2                                       # win_first of the three one-window sets
    assert 5162220 * 13 == 4 * ((1 << 24) - 1)
    cases = [(SP.FIR, SP.F32, SP.VAR_UNIT, ((1 << 23) - 2) // 3, 96, static, delta, 1, SP.K_FIR),
             (SP.CHUNK, SP.F64, SP.VAR_FRAME, (1 << 25) - 1, 8, ext2, static, 1, SP.K_CHUNK),
             (SP.CHUNK, SP.F64, SP.VAR_FRAME, 5162220, 256, ext2, static, 1, SP.K_CHUNK),
             (SP.GENERIC, SP.F64, SP.VAR_FRAME, (1 << 24) - 1, 256, static, static, 2, SP.K_GENERIC)]
    for algo, dtype, var_mode, B_most, T, w0, w1, sd1, kind in cases:
        name = "MLPG_HIP_ALGO_" + SP.ALGO_NAME[algo]
        tab = (StreamDesc * 2)(StreamDesc(0, 0, 1, 1, w0), StreamDesc(1, 1, sd1, 1, w1))
        ws0, ws1 = SP.Win(wl, wl, wc, w0, 1), SP.Win(wl, wl, wc, w1, 1)
        for B, refused in ((B_most, 1), (B_most + 1, 0)):
            rc = L.mlpg_hip_forward_streams(0, None, dtype, algo, fake, fake, var_mode, 1 + sd1, None, B, T, 2, ctypes.addressof(tab), 3,
                                            p(wl), p(wl), p(wc), fake, 1 + sd1, None)
            e = L.mlpg_hip_last_error().decode()
            assert rc == -1 and "stream %d: %s" % (refused, name) in e, (name, B, e)
            solo = lambda ws, sd: SP.solo_kind(None, ws, algo, var_mode, dtype, B, T, False, 1 + sd1, sd, False)  # noqa: E731
            if refused == 1:
                assert solo(ws0, 1) == kind, (name, B)
                with pytest.raises(SP.Refused) as ei:
                    solo(ws1, sd1)
            else:
                with pytest.raises(SP.Refused) as ei:
                    solo(ws0, 1)
            assert str(ei.value) == name
    # the predicates themselves, at the bound and one over
    w2 = SP.Win(wl, wl, wc, ext2, 1)
    assert SP.fir_workgroups(2796202, 96, 1) == (1 << 23) - 1 and SP.fir_grid_fits(2796202, 96, 1) and not SP.fir_grid_fits(2796203, 96, 1)
    assert SP.fir_grid_fits(2796202 // 2, 96, 128) and not SP.fir_grid_fits(2796202 // 2 + 1, 96, 128)    # two groups of dims
    assert SP.chunk_grid_fits((1 << 25) - 1, 8, 1, w2) and not SP.chunk_grid_fits(1 << 25, 8, 1, w2)
    assert SP.chunk_grid_fits(5162220, 256, 1, w2) and not SP.chunk_grid_fits(5162221, 256, 1, w2)
    assert SP.chunk_preferred(5162220, 256, 1, w2) and not SP.chunk_preferred(5162221, 256, 1, w2)          # AUTO goes elsewhere
    assert SP.generic_grid_fits((1 << 24) - 1, 256, 1) and not SP.generic_grid_fits(1 << 24, 256, 1)
    assert [L.mlpg_hip_launch_count(k) for k in range(44)] == c0

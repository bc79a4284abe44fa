"""The stream and workspace contract of the device entry points, as three checks that every family plugs into
(tests/test_stream_contract_gpu.py holds the table of cells, tests/test_workspace_content_gpu.py the workspace cells).

A cell is four callables around one dict of device tensors, ``bufs``:

``make(seed)``          the host side of one case, always at the cell's one fixed shape: two seeds give the same shapes, other values
                        and other lengths.
``load(bufs, case)``    brings the case into ``bufs`` through ``put`` / ``out``: the first load allocates, every later one copies in
                        place, lengths included, so that a captured graph sees the new data behind the same pointers.  Keys that
                        begin with ``in_`` are inputs the entry reads (``in_idx_``: indices it follows), keys that begin with
                        ``out_`` are tensors it writes.
``call(bufs)``          the wrapper call or calls.  Tensors a wrapper allocates itself are stored under ``out_`` keys, so that they
                        stay alive between a capture and its replays.
``verdict(case, bufs)`` the family's existing check against its model: the texts of what fails, or an assertion.

and a fifth that runs without a device, ``expected(case)``: the model's outputs as numpy arrays, for the conditions on a case pair
(``pair_conditions``).  Comparisons of one run with another run of the same entry are by bytes."""
import numpy as np

POISON = 0xA5      # the byte every output holds before a replay, and every input before its late producer (tests/silence_cases.py's)


class Cell(object):
    """One entry of the table: name, the four callables, ``expected`` and what the entry documents about capture."""

    def __init__(self, name, entries, make, load, call, verdict, expected, capture=True, why=None, poison=POISON, sentinel=None,
                 documented_by=None, defined=None):
        self.name, self.entries = name, tuple(entries)
        self.defined = defined          # defined(bufs) -> {name: array}: what one run is compared with another in, where an entry leaves
        #                                 part of an output unspecified (default: every byte of every input and output)
        self.documented_by = documented_by or (self.entries[0] if self.entries else None)      # the wrapper whose docstring `why` quotes
        self.make, self.load, self.call, self.verdict, self.expected = make, load, call, verdict, expected
        # poison: the byte the outputs are filled with; sentinel: the VALUE instead, for the families whose verdict expects one
        self.capture, self.why, self.poison, self.sentinel = capture, why, poison, sentinel
        assert capture or why, "%s: an entry kept out of capture quotes the sentence that documents why" % name

    def __repr__(self):
        return self.name


def _torch():
    import torch
    return torch


def put(bufs, key, array, device="cuda"):
    """bufs[key] holds ``array``: allocated by the first load, copied in place by every later one.  None stays None."""
    torch = _torch()
    if array is None:
        assert bufs.get(key) is None
        bufs[key] = None
        return None
    src = torch.from_numpy(np.ascontiguousarray(array))
    t = bufs.get(key)
    if t is None:
        t = bufs[key] = torch.empty(src.shape, dtype=src.dtype, device=device)
    assert t.shape == src.shape and t.dtype == src.dtype, (key, tuple(t.shape), tuple(src.shape), t.dtype, src.dtype)
    t.copy_(src)
    return t


def out(bufs, key, shape, dtype, device="cuda"):
    """bufs[key]: an output the caller owns, allocated by the first load and left as it is by later ones."""
    torch = _torch()
    if bufs.get(key) is None:
        bufs[key] = torch.empty(tuple(shape), dtype=dtype, device=device)
    return bufs[key]


def _tensors(bufs, prefix):
    torch = _torch()
    return [(k, v) for k, v in sorted(bufs.items()) if k.startswith(prefix) and torch.is_tensor(v)]


def fill_bytes(t, byte):
    """Every byte of a dense tensor set to ``byte`` on the current stream."""
    torch = _torch()
    assert t.is_contiguous()
    if t.numel():
        t.reshape(-1).view(torch.uint8).fill_(byte)


def poison_tensor(cell, t):
    """The family's poison: its byte in every byte, or its sentinel value in every element (-7 is 249 in a uint8 tensor)."""
    if cell.sentinel is None:
        fill_bytes(t, cell.poison)
    else:
        t.fill_(cell.sentinel % 256 if t.dtype == _torch().uint8 else cell.sentinel)


def poison_outputs(cell, bufs):
    for _, t in _tensors(bufs, "out_"):
        poison_tensor(cell, t)


def load_poisoned(cell, bufs, case):
    cell.load(bufs, case)
    poison_outputs(cell, bufs)


def snapshot(bufs):
    """The bytes of every input and output in ``bufs`` on the host (inputs too: an entry that writes one in place is compared
    there, one that must not is caught)."""
    torch = _torch()
    snap = {}
    for k, t in _tensors(bufs, "in_") + _tensors(bufs, "out_"):
        snap[k] = (str(t.dtype), tuple(t.shape), t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    return snap


def state(cell, bufs):
    return cell.defined(bufs) if cell.defined is not None else snapshot(bufs)


def differing(a, b):
    """The keys at which two snapshots differ."""
    def same(u, v):
        if isinstance(u, np.ndarray) and isinstance(v, np.ndarray):
            return u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()
        return u == v
    return sorted(k for k in set(a) | set(b) if k not in a or k not in b or not same(a[k], b[k]))


def check(cell, case, bufs, what):
    fails = cell.verdict(case, bufs)
    assert not fails, "%s, %s: %s" % (cell.name, what, fails)


# ---- the three checks ----------------------------------------------------------------------------------------------------------------

def replayed_on_new_data(cell, seed_a=1, seed_b=2):
    """``call`` captured once on a side stream with case A in the buffers, replayed with case B and then with A again behind the
    same pointers, every output filled with the poison byte before each replay.  Under capture a synchronisation or an allocation
    of the entry's own raises, a launch sent to another stream is not recorded (the poison stays), and whatever the host read
    from device data at capture time shows on the replay with B.  The capture is linear; nothing runs on the side stream between
    capture and replay but the replays themselves."""
    torch = _torch()
    A, B = cell.make(seed_a), cell.make(seed_b)
    bufs = {}
    load_poisoned(cell, bufs, A)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cell.call(bufs)                       # warm-up: tables and the library's scratch exist before the capture
    torch.cuda.synchronize()
    check(cell, A, bufs, "the eager warm-up on the side stream")
    first = state(cell, bufs)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        cell.call(bufs)
    torch.cuda.synchronize()
    for case, name in ((B, "B"), (A, "A again")):
        load_poisoned(cell, bufs, case)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(cell, case, bufs, "the replay on case %s" % name)
    assert differing(state(cell, bufs), first) == [], "the replay on A differs from the eager run on A in %s" % differing(state(cell, bufs), first)
    del g


def two_streams_interleaved(cell, seed_a=1, seed_b=2, rounds=8):
    """Case A on one stream and case B on another, eight rounds enqueued alternately with no synchronisation in between: both must
    give the bytes the default stream gave, and pass the verdict.  State shared across streams -- a table, scratch, a workspace
    keyed by device alone -- shows here."""
    torch = _torch()
    cases = (cell.make(seed_a), cell.make(seed_b))
    bufs = ({}, {})
    want = []
    for case, b in zip(cases, bufs):
        load_poisoned(cell, b, case)
        cell.call(b)
        torch.cuda.synchronize()
        check(cell, case, b, "the default stream")
        want.append(state(cell, b))
    for case, b in zip(cases, bufs):
        load_poisoned(cell, b, case)
    torch.cuda.synchronize()
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    for _ in range(rounds):
        for s, b in zip(streams, bufs):
            with torch.cuda.stream(s):
                cell.call(b)
    torch.cuda.synchronize()
    for case, b, w, name in zip(cases, bufs, want, "AB"):
        check(cell, case, b, "case %s after %d interleaved rounds" % (name, rounds))
        diff = differing(state(cell, b), w)
        assert diff == [], "case %s: the interleaved result differs from the default stream's in %s" % (name, diff)


def one_stream_shared(cells, seed=1):
    """The calls of several cells -- other entries, other shapes -- enqueued back to back on ONE side stream, in order and then in
    reverse, with no synchronisation inside a pass: every result passes its verdict and the two passes agree byte for byte.  The
    library's scratch belongs to a (device, stream): entries that share a slot, and calls of other shapes that grow it, meet
    here; a table or a control word that one call leaves behind and the next one trusts shows as a wrong or a changed result."""
    torch = _torch()
    runs = []
    for cell in cells:
        case, bufs = cell.make(seed), {}
        load_poisoned(cell, bufs, case)
        runs.append((cell, case, bufs))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    states = []
    for order in (runs, runs[::-1]):
        for cell, case, bufs in order:
            poison_outputs(cell, bufs)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for cell, case, bufs in order:
                cell.call(bufs)
        torch.cuda.synchronize()
        for cell, case, bufs in order:
            check(cell, case, bufs, "among %d calls on one stream" % len(runs))
        states.append({cell.name: state(cell, bufs) for cell, case, bufs in order})
    for cell, _, _ in runs:
        diff = differing(states[0][cell.name], states[1][cell.name])
        assert diff == [], "%s: the two passes differ in %s" % (cell.name, diff)


_SLEEP = {}


def sleep_cycles(ms=5.0):
    """The argument of torch.cuda._sleep that keeps a stream busy for about ``ms`` milliseconds, from torch.cuda.Event timing of
    the sleep itself."""
    torch = _torch()
    dev = torch.cuda.current_device()
    if dev not in _SLEEP:
        probe = 2000000
        torch.cuda._sleep(probe)              # (the first launch pays for loading the kernel)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        torch.cuda._sleep(probe)
        t1.record()
        torch.cuda.synchronize()
        _SLEEP[dev] = probe / max(t0.elapsed_time(t1), 1e-3)       # cycles per millisecond
    return int(min(_SLEEP[dev] * ms, 2e9))


def behind_a_late_producer(cell, seed=1):
    """On a side stream: the inputs filled with the poison byte, a sleep of a few milliseconds, in-place copies that bring the real
    inputs in, then ``call``; only that stream is synchronised.  An entry that launched on another stream, or read an input on the
    host, meets the poison.  The check can pass wrongly -- when the sleep is too short for the stray work to overtake the copies --
    and can never fail wrongly: on the stream it was handed, the entry runs behind the copies."""
    torch = _torch()
    case = cell.make(seed)
    bufs = {}
    load_poisoned(cell, bufs, case)
    torch.cuda.synchronize()
    staged = [(k, t, t.clone()) for k, t in _tensors(bufs, "in_")]
    cycles = sleep_cycles()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for k, t, _ in staged:
            if k.startswith("in_idx_"):
                t.zero_()                      # indices the kernel follows: wrong but in bounds, whatever stream reads them
            else:
                poison_tensor(cell, t)
        torch.cuda._sleep(cycles)
        for _, t, real in staged:
            t.copy_(real, non_blocking=True)
        cell.call(bufs)
    side.synchronize()
    check(cell, case, bufs, "behind a late producer")
    torch.cuda.synchronize()


# ---- the conditions on a case pair (no device) -------------------------------------------------------------------------------------------

def holds_poison(cell, a):
    """True where an element of ``a`` is what poison_tensor writes."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return False
    if cell.sentinel is not None:
        return bool((a == (cell.sentinel % 256 if a.dtype == np.uint8 else cell.sentinel)).any())
    raw = a.view(np.uint8).reshape(a.size, a.dtype.itemsize)
    return bool((raw == cell.poison).all(axis=1).any())


def pair_conditions(cell, seed_a=1, seed_b=2):
    """The texts of what keeps a case pair from telling a stale replay from a fresh one: an output that A and B share, an output
    in which the poison pattern is a legitimate value."""
    ea, eb = cell.expected(cell.make(seed_a)), cell.expected(cell.make(seed_b))
    assert len(ea) == len(eb) and len(ea) > 0
    fails = []
    for i, (a, b) in enumerate(zip(ea, eb)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (cell.name, i, a.shape, b.shape)
        if a.tobytes() == b.tobytes():
            fails.append("output %d is the same for A and B" % i)
        if holds_poison(cell, a) or holds_poison(cell, b):
            fails.append("output %d holds the poison pattern" % i)
    return fails

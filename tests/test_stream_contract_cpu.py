"""What keeps the stream-contract tests complete and sharp, checked without a GPU.

Completeness: the syntax trees of ``nnmnkwii_amd/_hip.py`` and the ``_*_hip.py`` bindings are walked for every function that asks
for the current stream (a call of ``_stream``); each must be named by a cell of tests/test_stream_contract_gpu.py's table or by
its ``COVERED_ELSEWHERE``, whose targets must exist.  A wrapper added later cannot escape the contract tests unnoticed.

Sharpness: for every cell, the model's outputs of case A and case B differ in every tensor (a stale replay cannot pass) and hold
the poison pattern nowhere (an output that was never written cannot pass); a cell kept out of the capture check quotes a sentence
of its wrapper's own docstring."""
import ast
import glob
import os

import pytest

import stream_contract as SC
import test_stream_contract_gpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nnmnkwii_amd")


def _tree(path):
    with open(path) as f:
        return ast.parse(f.read(), path)


def _functions(node, prefix=""):
    """(qualified name, FunctionDef) of every function and method below `node`."""
    for child in ast.iter_child_nodes(node):
        if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
            yield prefix + child.name, child
            yield from _functions(child, prefix + child.name + ".")
        elif isinstance(child, ast.ClassDef):
            yield from _functions(child, prefix + child.name + ".")


def _asks_for_the_stream(fn):
    for node in ast.walk(fn):
        if isinstance(node, ast.Call):
            f = node.func
            if (isinstance(f, ast.Name) and f.id == "_stream") or (isinstance(f, ast.Attribute) and f.attr == "_stream"):
                return True
    return False


def binding_functions():
    """{"module.function": FunctionDef} over the binding modules."""
    paths = [os.path.join(PKG, "_hip.py")] + sorted(glob.glob(os.path.join(PKG, "_*_hip.py")))
    return {"%s.%s" % (os.path.splitext(os.path.basename(path))[0], name): fn for path in paths for name, fn in _functions(_tree(path))}


FUNCTIONS = binding_functions()
USERS = {name: fn for name, fn in FUNCTIONS.items() if name != "_hip._stream" and _asks_for_the_stream(fn)}
IN_TABLE = {entry: cell for cell in T.CELLS for entry in cell.entries}


def test_the_walk_finds_the_bindings():
    """The walk itself: the seven modules, and wrappers of every kind -- plain, a method, one that hands the stream on in a name."""
    modules = {k.split(".")[0] for k in USERS}
    assert modules == {"_hip", "_frontend_hip", "_silence_hip", "_joint_hip", "_f0_hip", "_wave_hip", "_metrics_hip"}
    for name in ("_hip.forward", "_hip.fastdtw_l2", "_hip.fastdtw_callable", "_hip._mse_workspace", "_joint_hip.Plan.count",
                 "_joint_hip.Plan.write", "_metrics_hip.metrics_batch", "_wave_hip.decode"):
        assert name in USERS, name
    assert "_hip._stream" not in USERS and "_hip.modspec_route" not in USERS and "_wave_hip.plan" not in USERS
    assert len(USERS) >= 44


@pytest.mark.parametrize("name", sorted(USERS))
def test_every_wrapper_that_takes_the_stream_is_covered(name):
    assert (name in IN_TABLE) != (name in T.COVERED_ELSEWHERE), \
        "%s passes the current stream to the library: give it a cell in tests/test_stream_contract_gpu.py (or, where a stream or " \
        "capture test of its own exists, an entry of COVERED_ELSEWHERE) -- and not both" % name


def test_the_table_names_only_wrappers_that_exist():
    assert sorted(set(IN_TABLE) - set(USERS)) == [] and sorted(set(T.COVERED_ELSEWHERE) - set(USERS)) == []
    assert len({c.name for c in T.CELLS}) == len(T.CELLS)


@pytest.mark.parametrize("name", sorted(T.COVERED_ELSEWHERE))
def test_the_targets_of_covered_elsewhere_exist(name):
    path, test = T.COVERED_ELSEWHERE[name].split("::")
    assert path.startswith("tests/test_") and path.endswith("_gpu.py")
    full = os.path.join(ROOT, *path.split("/"))
    assert os.path.exists(full), path
    found = [fn for qual, fn in _functions(_tree(full)) if qual == test]
    assert len(found) == 1, (path, test)
    # the target is a stream test: it names a stream or a graph of torch.cuda
    names = {n.attr for n in ast.walk(found[0]) if isinstance(n, ast.Attribute)}
    assert names & {"Stream", "CUDAGraph", "graph"}, (path, test)


@pytest.mark.parametrize("cell", T.CELLS, ids=[c.name for c in T.CELLS])
def test_case_pairs_tell_a_stale_replay_from_a_fresh_one(cell):
    assert SC.pair_conditions(cell) == []


def test_the_joint_cases_sit_on_both_sides_of_the_capacity():
    import joint_cases as JC
    kept = [len(JC.expected(T.joint_case(seed))[0]) for seed in (1, 2)]
    assert kept[0] < T.JOINT_CAP < kept[1], kept


def test_a_cell_kept_out_of_capture_quotes_its_wrapper():
    out = [c for c in T.CELLS if not c.capture]
    assert sorted(c.name for c in out) == ["fastdtw_callable", "modspec_loss_step[n=64]"]
    for c in out:
        doc = " ".join((ast.get_docstring(FUNCTIONS[c.documented_by]) or "").split())
        assert " ".join(c.why.split()) in doc, (c.name, c.why)

"""GPU tests (-m gpu): nnmk_sil_frame_counts, nnmk_sil_expand and nnmk_sil_gather on buffers at odd element offsets between guard
bands (tests/embed.py, through tests/silence_cases.py: run_entries).  The phone matrix, the durations, the flags, num_phones and
len_src, the scaling vectors and the three outputs each start an odd number of elements into a byte buffer filled with one value --
the flags, one byte each, at any byte offset -- and after the calls the inputs hold their bits, every guard holds its fill byte,
the foreign columns of the outputs hold theirs, and counts, lengths and rows equal tools/silence_model.py bit for bit."""
import numpy as np
import pytest

import silence_cases as SC
from silence_cases import FM

pytestmark = pytest.mark.gpu

OFFSETS = [(1, 3, 1, 1, 1, 3), (3, 1, 5, 3, 1, 1), (5, 7, 2, 1, 3, 5), (1, 1, 7, 5, 1, 7)]


@pytest.mark.parametrize("offs", OFFSETS, ids=["-".join(map(str, o)) for o in OFFSETS])
@pytest.mark.parametrize("plans", [SC.PLANS_A, SC.PLANS_B], ids=["A", "B"])
def test_offset_buffers_between_guard_bands(plans, offs):
    i = sum(offs)
    T = SC.all_counts(plans)
    Tmax = int(T.max()) + 70
    lens = np.minimum(T + np.array([70, -1, 0, 5, -30, 0]), Tmax)
    for kind, S, dur, p_dtype, out_dtype, D in ((FM.FULL, 5, np.float32, np.float32, np.float64, 65), (FM.COARSE_CODING, 1, np.int64, np.float64, np.float32, 1),
                                                 (FM.NONE, 5, np.int32, np.float32, np.float32, 3)):
        P, d, sil, n, _ = SC.make_batch(i + S, plans, S, 62, dur)
        g = dict(Y=SC.source(i, len(plans), Tmax, D, np.clip(lens, 0, Tmax), p_dtype), len=lens)
        SC.run_entries(P, d, sil, n, kind, 0, kind != FM.NONE, p_dtype, out_dtype, gather=g, pad_p=1, pad_out=1, offs=offs, seed=i)

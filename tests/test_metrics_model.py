"""tools/metrics_model.py against itself and against the reference (-m "not gpu"): the literal per-utterance definition, the
kernel's partition and summation order, and the extended-precision truth on random ragged batches; the kernel order against the
values the reference gave (tests/golden/metrics_ref.npz).  The tolerances are the model's own: (longest addition chain + 4) 2^-53
against the truth, twice that against another float64 summation order."""
import numpy as np
import pytest

import metrics_cases as C
from metrics_cases import MM

BLOCK = C.BLOCK
G = C.golden()


@pytest.mark.parametrize("seed,lengths,Tmax", [(1, [BLOCK + 1], BLOCK + 1), (2, [0, 1, BLOCK - 1], BLOCK), (3, [5, 2 * BLOCK + 3, 0, BLOCK, 77], 2 * BLOCK + 3)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_literal_kernel_order_and_truth_agree(seed, lengths, Tmax, dtype):
    terms = C.eight_terms()
    X, Y, L = C.kernel_case(seed, lengths, Tmax, 187, dtype, dtype, terms)
    B = len(lengths)
    per, tot = MM.kernel_order(X, Y, L, terms)
    lit = MM.literal(X, Y, L, terms)
    t_per, t_tot = MM.truth(X, Y, L, terms)
    for i, t in enumerate(terms):
        rel = MM.bound(B, Tmax, t)
        assert np.array_equal(per[:, i, 1], lit[:, i, 1]) and np.array_equal(per[:, i, 1], t_per[:, i, 1])      # counts: exact
        assert tot[i, 1] == t_tot[i, 1] == lit[:, i, 1].sum()
        assert C.close(per[:, i, 0], t_per[:, i, 0], rel) and C.close(tot[i, 0], t_tot[i, 0], rel)
        assert C.close(lit[:, i, 0], per[:, i, 0], 2 * rel)                                                      # another order
        assert C.close(lit[:, i, 0], t_per[:, i, 0], rel)
    assert np.array_equal(per[np.asarray(lengths) == 0], np.zeros((lengths.count(0), 8, 2)))


def test_per_utterance_bits_do_not_depend_on_the_batch():
    terms = C.eight_terms()
    X, Y, L = C.kernel_case(4, [5, 2 * BLOCK + 3, 0, BLOCK, 77], 2 * BLOCK + 3, 140, np.float64, np.float64, terms)
    per, _ = MM.kernel_order(X, Y, L, terms)
    for b in (0, 3, 4):
        n = int(L[b])
        alone, tot = MM.kernel_order(X[b:b + 1, :n], Y[b:b + 1, :n], None, terms)
        assert np.array_equal(alone[0].view(np.int64), per[b].view(np.int64)) and np.array_equal(tot, alone[0])


def test_chain_lengths():
    t = MM.term(MM.SQUARED, 0, width=129)
    # 64 frames of a wave x 3 steps of a lane, the butterfly, the waves, 3 blocks, 1 utterance per segment, the tree
    assert MM.chain(5, 2 * BLOCK + 3, t) == 64 * 3 + 6 + 3 + 3 + 1 + 8
    assert MM.chain(513, 1, MM.term(MM.FRAME_L2, 0, width=59)) == (1 + 6) + 1 + 6 + 3 + 1 + 3 + 8
    assert MM.bound(1, 1, MM.term(MM.VOICED_SQUARED, 0, flags=MM.FLAG_EXP)) == (1 + 6 + 3 + 1 + 1 + 8 + 4 + 84) * 2.0 ** -53


@pytest.mark.parametrize("name", sorted(C.G_CASES))
def test_kernel_order_against_the_reference(name):
    X, Y, L = G[name + "/X"], G[name + "/Y"], G[name + "/lengths"]
    terms = C.golden_terms()
    _, tot = MM.kernel_order(X, Y, L, list(terms.values()))
    for i, (key, t) in enumerate(terms.items()):
        want = float(G["%s/%s" % (name, key)])
        rel = C.reference_bound(len(L), X.shape[1], t, X.dtype) + 3 * C.U      # the figure's own division, root and scaling
        got = C.figure(key, tot[i])
        print(name, key, got, want, abs(got - want) / want / rel)
        assert C.close(got, want, rel)
    # the same figures through the forms without lengths: one utterance is a batch of one
    u, n = 3, int(L[3])
    for key, t in (("melcd/utterance", terms["melcd/lengths"]), ("mse/utterance", terms["mse/lengths"]),
                   ("lf0/utterance", terms["lf0/lengths"]), ("lf0/utterance_linear", terms["lf0/lengths_linear"]),
                   ("vuv/utterance", terms["vuv/lengths"])):
        _, tot = MM.kernel_order(X[u:u + 1, :n], Y[u:u + 1, :n], None, [t])
        assert C.close(C.figure(key, tot[0]), float(G["%s/%s" % (name, key)]), C.reference_bound(1, n, t, X.dtype) + 3 * C.U)

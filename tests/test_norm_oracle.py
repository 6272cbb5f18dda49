"""The C oracle's torch.norm (oracle/uq_oracle.c: uqo_torch_norm2, the checker of the GPU's
KE2 / KE2s and of DRIVE's KR4) against torch.norm itself on CPU and the NumPy restatement
(oracle/uq_eden.py), on the adversarial vectors of tests/norm_cases.py."""
import numpy as np
import torch

from oracle import uq_eden as E
from oracle import uq_oracle_c as C
from tests.norm_cases import norm_cases, same_bits

# DRIVE takes torch.norm of an unpadded last chunk (AS:741): every length through nine 8-wide
# vectors (each L % 8, with and without the 4-wide step), and the ragged ends of a 2048 chunk
RAGGED_L = tuple(range(1, 73)) + (1025, 2043, 2044, 2045, 2046, 2047)


def test_c_norm_matches_torch_and_numpy_oracle():
    for D in (1, 2, 4, 8, 64, 1024, 16384):   # EDEN pads to powers of two
        for name, v in norm_cases(D):
            t = np.float32(torch.norm(torch.from_numpy(v), 2).item())
            c = C.torch_norm2(v)
            assert same_bits(c, t), (D, name, c, t)
            if D <= 1024:
                assert same_bits(c, E.torch_norm2(v)), (D, name)


def test_norm_of_every_ragged_length_matches_torch():
    """The tail after the whole 8-wide vectors: 4 elements by mul + add when 4 remain, the last
    1 to 3 by fma.  Both restatements against live torch.norm, bit for bit."""
    with np.errstate(all="ignore"):
        for L in RAGGED_L:
            cases = norm_cases(L)
            assert len(cases) == 16 and all(v.shape == (L,) and v.dtype == np.float32 for _, v in cases)
            for name, v in cases:
                t = np.float32(torch.norm(torch.from_numpy(v), 2).item())
                c = C.torch_norm2(v)
                assert same_bits(c, t), (L, name, c, t)
                e = E.torch_norm2(v)
                assert same_bits(e, t), (L, name, e, t)


def test_norm_cases_are_well_formed_at_small_lengths():
    """norm_cases' edits index with D // 2, D // 3, D // 5 and D - 9: in range at every length,
    and the NaN / Inf cases hold their NaN / Inf."""
    for L in (1, 2, 3, 4, 5, 8, 9, 10):
        d = dict(norm_cases(L))
        assert np.isnan(d["nan"]).sum() == 1 and np.isinf(d["inf"]).sum() == 1
        assert np.count_nonzero(d["single"]) == 1
        assert not d["zeros"].any()

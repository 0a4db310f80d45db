"""Host side of the kept-cache row selection (include/ivg.h ivg_kv_select), no GPU: ``stable_parents`` over exhaustive
small cases, the normalisation of ``parents``, the binding table, and the refusals of the C entries that come before any device work."""

import ctypes as C
import itertools
from collections import Counter

import numpy as np
import pytest
import torch

from ivideogpt_amd.transformer import normalize_parents, stable_parents


def test_stable_parents_exhaustive():
    """Every parents map with B <= 4 rows and n <= 5 children: the same multiset, ``arranged == parents[perm]`` with ``perm`` a
    permutation, and as many fixed points as any arrangement can have -- one per distinct value below n."""
    cases = 0
    for B in range(1, 5):
        for n in range(1, 6):
            for parents in itertools.product(range(B), repeat=n):
                arranged, perm = stable_parents(list(parents), B)
                assert arranged.dtype == torch.int64 and perm.dtype == torch.int64 and arranged.shape == perm.shape == (n,)
                a, q = arranged.tolist(), perm.tolist()
                assert sorted(q) == list(range(n)), (parents, q)
                assert a == [parents[j] for j in q] and Counter(a) == Counter(parents)
                fixed = sum(a[i] == i for i in range(n))
                assert fixed == len({v for v in parents if v < n}), (parents, a)     # (an arrangement has at most one fixed point per value)
                # hence every moved row copies from a row that stays or is dropped: direct moves only
                assert all(a[i] == i or a[i] >= n or a[a[i]] == a[i] for i in range(n)), (parents, a)
                # the first copy of every surviving value sits in the value's own row; the other entries keep their original order
                first = {v: parents.index(v) for v in set(parents) if v < n}
                assert all(q[v] == j for v, j in first.items()), (parents, q)
                free = [q[i] for i in range(n) if i not in first]
                assert free == sorted(free), (parents, q)
                cases += 1
    assert cases > 1000


def test_stable_parents_examples():
    arranged, perm = stable_parents([2, 2, 0], 3)
    assert arranged.tolist() == [0, 2, 2] and perm.tolist() == [2, 1, 0]
    arranged, perm = stable_parents(torch.tensor([3, 1, 1, 3]), 4)
    assert arranged.tolist() == [1, 1, 3, 3] and perm.tolist() == [2, 1, 3, 0]
    arranged, perm = stable_parents(np.array([0, 1, 2], dtype=np.int16), 3)
    assert arranged.tolist() == [0, 1, 2] and perm.tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        stable_parents([0, 3], 3)


@pytest.mark.parametrize("parents", [[1, 0, 1], (2,), np.array([1, 0, 1], dtype=np.int64), np.array([1, 0, 1], dtype=np.uint8),
                                     torch.tensor([1, 0, 1]), torch.tensor([1, 0, 1], dtype=torch.int32), torch.tensor([9, 1, 9, 0, 9, 1])[1::2]],
                         ids=["list", "tuple", "int64", "uint8", "tensor", "int32 tensor", "strided tensor"])
def test_parents_are_normalised(parents):
    p = normalize_parents(parents)
    assert isinstance(p, np.ndarray) and p.dtype == np.int32 and p.ndim == 1 and p.flags["C_CONTIGUOUS"]
    assert p.tolist() == [int(x) for x in parents]


@pytest.mark.parametrize("parents,rows", [([], None), ([[0, 1]], None), (0, None), ([0.0, 1.0], None), ([True, False], None), (["0"], None),
                                          (torch.tensor([0.0]), None), (torch.tensor([True]), None), (torch.zeros(0, dtype=torch.int64), None),
                                          (torch.zeros(2, 2, dtype=torch.int64), None), ([0, -1], None), ([0, 2 ** 31], None), ([0, 3], 3),
                                          (np.array([3]), 3)])
def test_bad_parents_raise_value_error(parents, rows):
    with pytest.raises(ValueError):
        normalize_parents(parents, rows)


def test_binding_table_has_the_new_entries():
    from ivideogpt_amd import _lib
    l = _lib.load()
    for name, n_args in (("ivg_kv_select", 4), ("ivg_cache_select", 6), ("ivg_op_kv_select", 14)):
        res, args = _lib.EXPORTS[name]
        assert res is C.c_int and len(args) == n_args and hasattr(l, name)
    c0 = (l.ivg_debug_counter(b"kv_select_direct"), l.ivg_debug_counter(b"kv_select_staged"))
    assert min(c0) >= 0 and l.ivg_debug_counter(b"kv_select") == -1
    # refusals that come before any device work (no GPU here): null handles and bad shapes
    p = (C.c_int32 * 2)(0, 1)
    assert l.ivg_kv_select(None, p, 2, None) == -1
    assert l.ivg_cache_select(None, None, p, 2, None, None) == -1
    assert l.ivg_op_kv_select(None, 2, 8, 2, 40, 16, 0, 1, 2, p, 2, None, 0, None) == -1
    buf = (C.c_char * 64)()
    for bad in (dict(ra=8), dict(rb=8), dict(length=0), dict(length=41), dict(chunk=129), dict(B_old=9), dict(n=0), dict(layers=0)):
        a = dict(layers=2, chunk=8, heads=2, Lmax=40, ra=16, rb=0, length=1, B_old=2, n=2)
        a.update(bad)
        assert l.ivg_op_kv_select(buf, a["layers"], a["chunk"], a["heads"], a["Lmax"], a["ra"], a["rb"], a["length"], a["B_old"], p, a["n"], None, 0, None) == -1, bad
    assert l.ivg_op_kv_select(buf, 2, 1, 2, 40, 16, 0, 1, 1, p, 2, None, 0, None) == -4, "n above the chunk"
    assert l.ivg_op_kv_select(buf, 2, 8, 2, 40, 16, 0, 1, 2, (C.c_int32 * 2)(0, 2), 2, None, 0, None) == -1, "an index outside the old rows"
    assert l.ivg_op_kv_select(buf, 2, 8, 2, 40, 16, 0, 1, 2, p, 2, None, 0, None) == 0, "the identity launches nothing (and touches nothing)"
    assert (l.ivg_debug_counter(b"kv_select_direct"), l.ivg_debug_counter(b"kv_select_staged")) == c0

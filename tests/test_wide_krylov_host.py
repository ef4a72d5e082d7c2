"""Option lanczos_wide_krylov and stat wide_krylov_projections (taken from reserved slots, ABI version unchanged), and the
host K x K eigensolvers at the Krylov dimensions of the wide Lanczos kernels (256..511).  No GPU needed."""
import ctypes

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B


def test_wide_krylov_option_default_by_name_and_layout():
    o = B.default_options()
    assert o.lanczos_wide_krylov == 0 and B.get_option(o, "lanczos_wide_krylov") == 0
    B.set_option(o, "lanczos_wide_krylov", 1)
    assert o.lanczos_wide_krylov == 1 and B.get_option(o, "lanczos_wide_krylov") == 1
    # the field took the first reserved slot: the offsets of everything around it and the struct sizes are unchanged
    assert B.Options.lanczos_wide_krylov.offset == B.Options.block_batch_groups.offset + 4
    assert B.Options.reserved_i2.offset == B.Options.lanczos_wide_krylov.offset + 4
    assert B.Options.full_eig_lanczos_warm_pow.offset == B.Options.lanczos_wide_krylov.offset + 32
    assert B.Stats.wide_krylov_projections.offset == B.Stats.dense_truncated_projections.offset + 8
    assert B.Stats.reserved_s.offset == B.Stats.wide_krylov_projections.offset + 8
    assert o.struct_size == ctypes.sizeof(B.Options)             # sizeof(proxsdp_options) on the C side
    assert B.lib().proxsdp_hip_abi_version() == 10
    assert "wide_krylov_projections" in [f[0] for f in B.Stats._fields_]


def _rq(D, f, al, be):
    K, m = len(al), len(D)
    T = np.zeros((K, K))
    T[np.arange(m), np.arange(m)] = D
    if m:
        T[m, :m] = f; T[:m, m] = f
    for k in range(m, K):
        T[k, k] = al[k]
        if k + 1 < K:
            T[k, k + 1] = T[k + 1, k] = be[k]
    return T


@pytest.mark.parametrize("K", [300, 401, 511])
def test_host_symeig_at_wide_krylov_dimensions(K):
    """The Rayleigh quotient of a wide run: plain tridiagonal (first cycle) and arrow + tail (after a restart), by the
    QL path (host_symeig, threaded and serial bit-identical) and by the split + merge path, against LAPACK."""
    rng = np.random.default_rng(K)
    al = rng.standard_normal(K) * 3
    be = np.abs(1 + 0.3 * rng.standard_normal(K))
    m = (3 * K) // 5
    D = np.sort(rng.uniform(1, 60, m))[::-1].copy()
    f = rng.standard_normal(m) * np.where(np.arange(m) < m // 3, 1e-13, 1e-2)
    al2 = np.zeros(K); be2 = np.zeros(K)
    al2[m:] = rng.standard_normal(K - m)
    be2[m:] = np.abs(1 + 0.1 * rng.standard_normal(K - m))
    for D_, f_, a_, b_, k1 in [(np.zeros(0), np.zeros(0), al, be, K // 2), (D, f, al2, be2, m + 1)]:
        T = _rq(D_, f_, a_, b_)
        ref = np.linalg.eigvalsh(T)
        sc = max(1.0, np.abs(T).max())
        d, U = B.host_symeig(T, threads=-1)
        d0, U0 = B.host_symeig(T, threads=0)
        assert np.array_equal(d, d0) and np.array_equal(U, U0)
        assert np.abs(np.sort(d) - ref).max() <= 1e-13 * K * sc
        assert np.abs(U.T @ U - np.eye(K)).max() <= 1e-12
        assert np.abs(T @ U - U * d).max() <= 1e-13 * K * sc
        ds, Us, info = B.host_symeig_split(D_, f_, a_, b_, k1)
        assert np.abs(ds - ref).max() <= 1e-13 * K * sc
        assert np.abs(Us.T @ Us - np.eye(K)).max() <= 1e-13
        d3, U3, info3 = B.host_symeig_split(D_, f_, a_, b_, k1, threads=3)
        assert np.array_equal(d3, ds) and np.array_equal(U3, Us) and info3 == info

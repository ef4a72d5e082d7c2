"""One damaged argument against every C entry that accepts it (csrc/capi.hip check_request): the three INVALID tables of
test_warm_start_host.py (proxsdp_start), test_solution_factors_host.py (proxsdp_psd_factors) and test_device_results_host.py
(proxsdp_device_vectors), and one driver that calls any solve entry on the same tiny model -- kat_problems.sdp_wiki(False),
one PSD cone of side 3 -- with well-formed arguments of every kind the entry accepts, one of them then damaged.

Nothing here needs a device for a REFUSED call: every case of the tables is decided on the host.  The fake device pointers
of the device-vector table are handed over only together with such a case; an undamaged call gets host arguments only, so
with a GPU it simply solves."""
import ctypes as C

import numpy as np

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd.binding import DeviceVectors

from kat_problems import sdp_wiki
from test_device_results_host import FAKE, INVALID as DEVICE_INVALID, _ptr
from test_solution_factors_host import INVALID as FACTORS_INVALID
from test_warm_start_host import INVALID as START_INVALID, _wiki_start

E_INVALID, E_HIP, E_UNSUPP = -1, -2, -4

# the request fields each entry accepts (a handle's solve: GPU only, tests/test_model_handle.py)
ACCEPTS = {
    "solve_factored": ("factors",),
    "solve_from": ("start", "factors"),
    "solve_device": ("start", "factors", "device"),
    "model_solve": ("start", "factors", "device"),
    "start_point": ("start",),
    "exit_vectors": (),
}
# at proxsdp_hip_solve_factored a NULL struct is an error (test_solution_factors_host keeps that case); everywhere else NULL
# means "no factors wanted", which is no damage
FACTORS_CASES = sorted(set(FACTORS_INVALID) - {"null_struct"})
START_CASES = sorted(START_INVALID)
DEVICE_CASES = sorted(DEVICE_INVALID)


def shard(M):
    """make the marshalled problem a shard of a block-sharded solve"""
    cb = B.REDUCE_FN(lambda ctx, ps, ns, pm, nm: 0)
    M.keep.append(cb)
    M.P.reduce_fn = C.cast(cb, C.c_void_p)


def request_call(entry, table=None, case=None, as_shard=False, handle=None):
    """(return code, last error) of `entry` on sdp_wiki.  table: None (nothing damaged), "start", "factors" or "device";
    case: a key of that table.  handle: the proxsdp_model* of a Model of sdp_wiki, for entry == "model_solve"."""
    L = B.lib()
    accepts = ACCEPTS[entry]
    assert table is None or table in accepts, (entry, table)
    pr, st = _wiki_start()
    M = B._Marshalled(pr)
    o = B.default_options()
    R = B.Result()
    res = [np.zeros(max(k, 1)) for k in (pr.n, pr.n, pr.p, pr.m, pr.p, pr.m)]
    R.primal, R.dual_cone, R.dual_eq, R.dual_in, R.slack_eq, R.slack_in = [B._p(a) for a in res]
    S = F = sd = od = None
    if table == "device":
        # as test_device_results_host._call: a start that leaves dual_eq / dual_in to the device, fake device pointers
        rng = np.random.default_rng(0)
        st = dict(primal=rng.standard_normal(pr.n), factors=[(np.array([2.0, 0.5]), rng.standard_normal((3, 2)))])
        S, sarr = B._start_struct(pr.n, pr.p, pr.m, B.psd_sides(pr), st)
        sd, od = DeviceVectors(), DeviceVectors()
        for v in (sd, od):
            v.struct_size = C.sizeof(DeviceVectors)
            v.device_id = o.device_id
        sd.dual_eq, sd.dual_in = _ptr(FAKE), _ptr(FAKE + 4096)
        od.primal, od.dual_cone = _ptr(FAKE + 8192), _ptr(FAKE + 12288)
        args = dict(S=S, arr=sarr, sd=sd, od=od, M=M, o=o, start=C.byref(S), start_dev=C.byref(sd), out_dev=C.byref(od))
        DEVICE_INVALID[case][0](args)
        S, sd, od = args["start"], args["start_dev"], args["out_dev"]
    else:
        if "start" in accepts:
            S, sarr = B._start_struct(pr.n, pr.p, pr.m, B.psd_sides(pr), st)
            if table == "start":
                START_INVALID[case](S, sarr, M)
            S = C.byref(S)
        if "factors" in accepts:
            F, farr = B._factors_struct(B.psd_sides(pr), True)
            if table == "factors":
                FACTORS_INVALID[case](F, farr, M)
            F = C.byref(F)
    if as_shard:
        shard(M)
    P = C.byref(M.P)
    if entry == "solve_factored":
        rc = L.proxsdp_hip_solve_factored(P, C.byref(o), C.byref(R), F)
    elif entry == "solve_from":
        rc = L.proxsdp_hip_solve_from(P, C.byref(o), C.byref(R), S, F)
    elif entry == "solve_device":
        rc = L.proxsdp_hip_solve_device(P, C.byref(o), C.byref(R), S, sd, F, od)
    elif entry == "model_solve":
        rc = L.proxsdp_hip_model_solve(handle, C.byref(o), C.byref(R), S, sd, F, od)
    elif entry == "start_point":
        T, tarr = B._state_struct(pr.n, pr.p + pr.m, 1, o.convergence_window)
        rc = L.proxsdp_hip_start_point(P, C.byref(o), S, C.byref(T))
    else:
        assert entry == "exit_vectors"
        x, y = np.zeros(pr.n), np.zeros(pr.p + pr.m)
        out = [np.zeros(max(k, 1)) for k in (pr.n, pr.n, pr.p, pr.m, pr.p, pr.m)]
        nneg = sum(len(v) for v in pr.psd)
        viol, neg = np.zeros(4), np.zeros(max(nneg, 1))
        rc = L.proxsdp_hip_exit_vectors(P, C.byref(o), B._p(x), B._p(y), 0, *[B._p(a) for a in out], B._p(viol), B._p(neg), nneg)
    return rc, L.proxsdp_hip_last_error().decode()

"""CPU-only tests of the one request check behind the C solve entries (csrc/capi.hip check_request): a damaged proxsdp_start,
proxsdp_psd_factors or proxsdp_device_vectors is refused with the same code at EVERY entry that accepts the argument, on the
host -- before a solver, and with it a device, exists (a call that got as far as the device would come back with
PROXSDP_E_HIP on a machine without one).  The tables are the ones the three features' own host tests run against their own
entry; the driver is solve_request_cases.request_call."""
import pytest

from proxsdp_jl_amd import binding as B

import solve_request_cases as Q
from solve_request_cases import E_HIP, E_INVALID, E_UNSUPP, request_call

HOST_ENTRIES = ("solve_factored", "solve_from", "solve_device", "start_point", "exit_vectors")


def _entries(table):
    return [e for e in HOST_ENTRIES if table in Q.ACCEPTS[e]]


def test_the_tables_reach_the_entries_the_issue_names():
    assert _entries("start") == ["solve_from", "solve_device", "start_point"]
    assert _entries("factors") == ["solve_factored", "solve_from", "solve_device"]
    assert _entries("device") == ["solve_device"]


@pytest.mark.parametrize("case", Q.START_CASES)
def test_a_malformed_start_is_refused_alike_at_every_entry_that_takes_one(case):
    for entry in _entries("start"):
        rc, msg = request_call(entry, "start", case)
        assert rc == E_INVALID, (case, entry, rc, msg)               # not PROXSDP_E_HIP: decided on the host
        assert msg, (case, entry)


@pytest.mark.parametrize("case", Q.FACTORS_CASES)
def test_malformed_factors_are_refused_alike_at_every_entry_that_takes_them(case):
    for entry in _entries("factors"):
        rc, msg = request_call(entry, "factors", case)
        assert rc == E_INVALID, (case, entry, rc, msg)
        assert msg, (case, entry)


@pytest.mark.parametrize("case", Q.DEVICE_CASES)
def test_malformed_device_vectors_are_refused_with_the_word_the_table_names(case):
    word = Q.DEVICE_INVALID[case][1]
    for entry in _entries("device"):
        rc, msg = request_call(entry, "device", case)
        assert rc == E_INVALID, (case, entry, rc, msg)
        assert word in msg, (case, entry, msg)


@pytest.mark.parametrize("entry", HOST_ENTRIES)
def test_a_shard_is_unsupported_at_every_entry(entry):
    rc, msg = request_call(entry, as_shard=True)
    assert rc == E_UNSUPP and "shard" in msg, (entry, rc, msg)


@pytest.mark.parametrize("entry", HOST_ENTRIES)
def test_the_undamaged_call_passes_the_host_checks(entry):
    """the control of every case above: with a GPU the call runs, without one it fails at the device and nowhere earlier"""
    rc, msg = request_call(entry)
    assert rc == (0 if B.device_count() > 0 else E_HIP), (entry, rc, msg)

"""GPU: argument errors of the nine parity-pass entry points (encode / verify /
locate, each from host pointers, as a strided device batch and as a mixed
device batch; maxio_amd/csrc/parity_pass.cpp), through ctypes.

Every case starts from one valid call over a 2+2 object of 64-byte shards
and changes one argument; the library answers before it launches anything,
except where a case says otherwise.  The codes are include/maxio_ec.h's."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import oracle
from maxio_amd import _native as N

pytestmark = pytest.mark.gpu

OK, E_FEW_DATA, E_FEW_PARITY, E_SHARD_SIZE, E_EMPTY, E_255, E_ARG = 0, -3, -5, -9, -11, -20, -21
POLICIES = ("encode", "verify", "locate")
FORMS = ("host", "strided", "batch")
K, M, S, PITCH, ROWS = 2, 2, 64, 256, 256  # ROWS: pointer tables long enough for k + m = 256
VERIFY_OK = (1 << 64) - 1


def _name(policy, form):
    return "mxec_" + policy + {"host": "", "strided": "_strided_device", "batch": "_batch_device"}[form]


@pytest.fixture(scope="module")
def mem():
    """Host and device rows of PITCH bytes (rows 0, 1: data; 2, 3: their
    parity) and a device result area."""
    import torch

    rng = np.random.default_rng(7200)
    host = np.zeros((ROWS, PITCH), np.uint8)
    host[:K, :S] = rng.integers(0, 256, (K, S), dtype=np.uint8)
    host[:K, S:] = 0xEE  # past the chunks: never read
    for i, p in enumerate(oracle.encode([host[j, :S] for j in range(K)], M, S)):
        host[K + i, :S] = p
    dev = torch.from_numpy(host).cuda()
    res = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return {"host": host, "dev": dev, "res": res}


def good(mem, policy, form):
    """The arguments of a valid call, by name."""
    base = mem["host"].ctypes.data if form == "host" else mem["dev"].data_ptr()
    a = {"k": K, "m": M, "S": S, "n_obj": 1, "dev": 0,
         "data_len": [S] * ROWS,
         "result": None if policy == "encode" else mem["res"].data_ptr()}
    if form == "strided":
        a.update(data=base, parity=base + K * PITCH)
    else:
        a.update(data=[base + j * PITCH for j in range(ROWS)],
                 parity=[base + (K + i) * PITCH for i in range(ROWS - K)] + [base] * K)
    if form == "host":
        a["first_bad"] = (ctypes.c_uint64 * ROWS)()
        a["consistent"] = ctypes.c_int(-1)
        a["result"] = N.LocateResult()
    return a


def call(ctx, policy, form, a):
    fn = getattr(N.lib(), _name(policy, form))

    def table(v, ct):
        return None if v is None else (ct * len(v))(*v)

    if form == "host":
        tail = {"encode": (None,),
                "verify": (a["first_bad"], ctypes.byref(a["consistent"]) if a["consistent"] is not None else None),
                "locate": (ctypes.byref(a["result"]) if a["result"] is not None else None,)}[policy]
        return fn(ctx.handle, a["k"], a["m"], a["S"], table(a["data"], ctypes.c_void_p),
                  table(a["data_len"], ctypes.c_size_t), table(a["parity"], ctypes.c_void_p), *tail)
    dl = table(a["data_len"], ctypes.c_uint64)
    if form == "strided":
        return fn(ctx.handle, a["dev"], None, a["k"], a["m"], a["S"], a["n_obj"], a["data"], 64 * PITCH, PITCH, dl,
                  a["parity"], 64 * PITCH, PITCH, a["result"])
    objs = None if a["n_obj"] == 0 else (N.Object * 1)(N.Object(a["k"], a["m"], a["S"]))
    return fn(ctx.handle, a["dev"], None, objs, a["n_obj"], table(a["data"], ctypes.c_void_p), dl,
              table(a["parity"], ctypes.c_void_p), a["result"])


def _first_null(a, key):
    return {key: [None] + a[key][1:]}


# (case, the forms it applies to, the policies, what it changes, the code)
ALL, DEVICE, LISTS = FORMS, ("strided", "batch"), ("host", "batch")
CASES = [
    ("k=0", ALL, POLICIES, lambda a: {"k": 0}, E_FEW_DATA),
    ("m=0", ALL, POLICIES, lambda a: {"m": 0}, E_FEW_PARITY),
    ("k+m=256", ALL, POLICIES, lambda a: {"k": 250, "m": 6}, E_255),
    ("m=1", ALL, ("locate",), lambda a: {"m": 1}, E_ARG),
    ("m=9", ALL, ("locate",), lambda a: {"m": 9}, E_ARG),
    ("shard_size=0", ALL, POLICIES, lambda a: {"S": 0}, E_EMPTY),
    ("n_obj=0,all-null", DEVICE, POLICIES,
     lambda a: {"n_obj": 0, "data": None, "parity": None, "data_len": None, "result": None}, OK),
    ("null-data", ALL, POLICIES, lambda a: {"data": None}, E_ARG),
    ("null-parity", ALL, POLICIES, lambda a: {"parity": None}, E_ARG),
    ("null-result", DEVICE, ("verify", "locate"), lambda a: {"result": None}, E_ARG),
    ("null-result", ("host",), ("locate",), lambda a: {"result": None}, E_ARG),
    # mxec_verify's two outputs are both optional: this one runs the pass
    ("null-result", ("host",), ("verify",), lambda a: {"first_bad": None, "consistent": None}, OK),
    ("one-null-data-pointer", LISTS, POLICIES, lambda a: _first_null(a, "data"), E_ARG),
    ("one-null-parity-pointer", LISTS, POLICIES, lambda a: _first_null(a, "parity"), E_ARG),
    ("data_len[0]=S+1", ("host",), POLICIES, lambda a: {"data_len": [S + 1] + [S] * (ROWS - 1)}, E_SHARD_SIZE),
    ("dev=count", DEVICE, POLICIES, lambda a: {"dev": -1}, E_ARG),  # -1: replaced by the context's device count
]
TABLE = [pytest.param(name, form, policy, change, code, id="%s-%s" % (_name(policy, form), name))
         for (name, forms, policies, change, code) in CASES for form in forms for policy in policies]


@pytest.mark.parametrize("name,form,policy,change,code", TABLE)
def test_argument_error(ctx, mem, name, form, policy, change, code):
    a = good(mem, policy, form)
    a.update(change(a))
    if a["dev"] == -1:
        a["dev"] = len(ctx.device_ids())
    assert call(ctx, policy, form, a) == code, N.lib().mxec_last_error()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("policy", POLICIES)
def test_the_valid_call_succeeds(ctx, mem, policy, form):
    """The call every case above starts from (this one launches)."""
    import torch

    a = good(mem, policy, form)
    assert call(ctx, policy, form, a) == OK, N.lib().mxec_last_error()
    torch.cuda.synchronize()
    if (policy, form) == ("verify", "host"):
        assert a["consistent"].value == 1 and list(a["first_bad"])[:M] == [VERIFY_OK] * M


@pytest.mark.parametrize("form", DEVICE)
def test_device_forms_clamp_a_long_data_len(ctx, mem, form):
    """data_len[0] = shard_size + 1 is clamped to shard_size by the device
    forms (the host forms refuse it, above): the encode writes the parity of
    the 64-byte chunks, and the verify and the locate find it consistent."""
    import torch

    dev, res = mem["dev"], mem["res"]
    dev[K:K + M].fill_(0)
    torch.cuda.synchronize()
    for policy in POLICIES:
        a = good(mem, policy, form)
        a["data_len"] = [S + 1] + [S] * (ROWS - 1)
        res.fill_(0x55)
        torch.cuda.synchronize()
        assert call(ctx, policy, form, a) == OK, (policy, N.lib().mxec_last_error())
        torch.cuda.synchronize()
        if policy == "encode":
            assert np.array_equal(dev[K:K + M, :S].cpu().numpy(), mem["host"][K:K + M, :S])
        elif policy == "verify":
            assert res[:8 * M].cpu().numpy().tobytes() == b"\xff" * (8 * M)
        else:
            rec = np.frombuffer(res[:24].cpu().numpy().tobytes(), "<u8,<u8,<u4,<u4")[0]
            assert (int(rec[0]), int(rec[1])) == (VERIFY_OK, 0)

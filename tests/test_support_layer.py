"""CPU: the test suite's own support layer.  Every module marked `gpu` carries the fault guard of tests/gpu_support.py, no module
under tests/ imports a test module, the guard ends the session on a sticky device error without ever being what opens the device
(checked with torch.cuda patched: nothing here runs a kernel), and the one FP8 row-quantiser of tests/fp8_ref.py gives the same
bytes, scales and x' whether a matrix goes in whole or row by row."""
import ast
import glob
import os

import pytest
import torch

import fp8_ref
import gpu_support

HERE = os.path.dirname(os.path.abspath(__file__))
MODULES = {os.path.basename(p)[:-3]: ast.parse(open(p).read()) for p in sorted(glob.glob(os.path.join(HERE, "*.py")))}


def _imports(tree):
    """(module, name or None) of every import statement, at any depth."""
    for n in ast.walk(tree):
        if isinstance(n, ast.Import):
            yield from ((a.name, None) for a in n.names)
        elif isinstance(n, ast.ImportFrom):
            yield from ((n.module or "", a.name) for a in n.names)


def _is_gpu_module(tree):
    return any(isinstance(n, ast.Assign) and [getattr(t, "id", None) for t in n.targets] == ["pytestmark"]
               and ast.unparse(n.value) == "pytest.mark.gpu" for n in tree.body)


def _is_fixture(fn):
    return any("fixture" in ast.unparse(d) for d in fn.decorator_list)


def test_every_gpu_module_imports_the_fault_guard():
    gpu = [m for m, t in MODULES.items() if m.startswith("test_") and _is_gpu_module(t)]
    assert len(gpu) >= 24
    for m in gpu:
        assert ("gpu_support", "stop_after_a_device_fault") in set(_imports(MODULES[m])), m


def test_no_module_imports_a_test_module():
    for m, tree in MODULES.items():
        bad = [mod for mod, _ in _imports(tree) if mod.split(".")[-1].startswith("test_")]
        assert not bad, (m, bad)


def test_the_library_fixture_and_the_guard_are_defined_once():
    for m, tree in MODULES.items():
        if m == "gpu_support":
            continue
        for n in ast.walk(tree):
            if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)):
                assert not (n.name == "B" and _is_fixture(n)), m
                assert "stop_after_a_device_fault" not in n.name, m
    own = {n.name for n in MODULES["gpu_support"].body if isinstance(n, ast.FunctionDef) and _is_fixture(n)}
    assert own == {"B", "stop_after_a_device_fault"}


def _teardown(monkeypatch, initialized, synchronize):
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: initialized)
    monkeypatch.setattr(torch.cuda, "synchronize", synchronize)
    guard = gpu_support.stop_after_a_device_fault.__wrapped__()
    next(guard)
    with pytest.raises(StopIteration):
        next(guard)


def test_the_guard_ends_the_session_on_a_sticky_error(monkeypatch):
    def synchronize():
        raise RuntimeError("HIP error: an illegal memory access was encountered")
    with pytest.raises(pytest.exit.Exception) as ei:
        _teardown(monkeypatch, True, synchronize)
    assert ei.value.returncode == 3 and "illegal memory access" in str(ei.value)


def test_the_guard_synchronises_an_open_device_and_never_opens_one(monkeypatch):
    calls = []
    _teardown(monkeypatch, True, lambda: calls.append(1))
    assert calls == [1]
    _teardown(monkeypatch, False, lambda: calls.append(2))
    assert calls == [1]


def test_importing_gpu_support_runs_nothing_but_definitions():
    """Collection runs where there is no device: at module level only the docstring, imports, DEV and the definitions."""
    body = MODULES["gpu_support"].body
    assert isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant)
    for n in body[1:]:
        assert isinstance(n, (ast.Import, ast.ImportFrom, ast.FunctionDef)) or ast.unparse(n) == "DEV = 'cuda'", ast.unparse(n)


def test_the_quantiser_is_the_same_over_a_matrix_and_over_its_rows():
    D = 64
    g = torch.Generator().manual_seed(11)
    mag = torch.exp2(torch.randint(-12, 5, (56, 1), generator=g).float())          # row magnitudes over 2^-12 .. 2^4
    w = torch.cat([fp8_ref.edge_rows(D), (torch.randn(56, D, generator=g) * mag).to(torch.bfloat16)])
    q, s, xp = fp8_ref.ref_q(w)
    assert q.shape == (64, D) and q.dtype == torch.uint8 and s.shape == (64,) and s.dtype == torch.float32 and xp.dtype == torch.bfloat16
    bits = lambda t: t.contiguous().view(torch.int16)
    for rows in (w.view(4, 16, D), w.view(2, 4, 8, D)):
        q2, s2, xp2 = fp8_ref.ref_q(rows)
        assert torch.equal(q2.reshape(64, D), q) and torch.equal(s2.reshape(64), s) and torch.equal(bits(xp2).reshape(64, D), bits(xp))
    for i in range(64):
        qi, si, xi = fp8_ref.ref_q(w[i])
        assert torch.equal(qi, q[i]) and torch.equal(si, s[i]) and torch.equal(bits(xi), bits(xp[i])), i
    # the contract on the edge rows: an all-zero row has scale 1, -0.0 keeps its sign bit, 448 * 2^e lands on the top code
    assert float(s[0]) == 1.0 and bool((q[0] == 0).all()) and float(s[4]) == 1.0 and bool((q[4] == 0x80).all())
    assert int(q[2, 7]) == 0x7E and float(s[2]) == 2.0 ** -3
    assert torch.equal(xp.double(), q.view(torch.float8_e4m3fn).double() * s.double()[:, None])      # x' = q * 2^e, exactly

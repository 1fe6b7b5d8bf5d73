"""The public surface of the standalone AMG V-cycle solver (no GPU): the two names pysolvers_amd.Linear was
missing (the reference's Linear/__init__.py line 11), their constructor signatures against the reference's —
recorded as data by tests/golden/make_vcycle.py — and the psk_vcycle entry point in header, library and binding."""
import ctypes
import inspect
import json
import os
import re

from conftest import GOLDEN, REPO


def _manifest():
    with open(os.path.join(GOLDEN, "manifest_vcycle.json")) as f:
        return json.load(f)


def test_names_are_exported():
    from pysolvers_amd.Linear import AMGVCycle, AMGVCycleSolver, IterativeLinearSolver, IterativeLinearSolverType
    assert issubclass(AMGVCycle, IterativeLinearSolverType)
    assert issubclass(AMGVCycleSolver, IterativeLinearSolver)


def _params(cls):
    out = []
    for p in list(inspect.signature(cls.__init__).parameters.values())[1:]:
        d = p.default
        if isinstance(d, (int, float, str)) or d is None:
            dd = dict(value=d)
        elif inspect.isclass(d):
            dd = dict(cls=d.__name__)
        else:
            dd = dict(instance_of=type(d).__name__)
        out.append(dict(name=p.name, default=dd))
    return out


def test_constructor_signatures_match_the_reference():
    from pysolvers_amd import Linear
    want = _manifest()["signatures"]
    assert sorted(want) == ["AMGVCycle", "AMGVCycleSolver"]
    for name, params in want.items():
        assert _params(getattr(Linear, name)) == params, name


def test_factory_passes_everything_through():
    from pysolvers_amd import CommonSolverArgs
    from pysolvers_amd.Linear import AMGVCycle, AMGVCycleSolver, JacobiSmoother
    ctl = CommonSolverArgs(maxiter=7, tau=1e-3)
    t = AMGVCycle(ctl, numLevels=3, nuPre=1, nuPost=4, smoother=JacobiSmoother)
    s = t.makeSolver(name="vc")
    assert isinstance(s, AMGVCycleSolver) and s.name() == "vc"
    assert (s.numLevels, s.nuPre, s.nuPost, s.smoother) == (3, 1, 4, JacobiSmoother)
    assert s.maxiter() == 7 and s.tau() == 1e-3 and not s.matrixFrozen()
    assert AMGVCycleSolver().name() == "AMGVCycle"
    # the reference's factory drops its own name (VCycleSolver.py:20): makeSolver() names the solver ''
    assert t.makeSolver().name() == t.name() == ""


def test_psk_vcycle_in_header_library_and_binding():
    from pysolvers_amd import _native as N
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "psk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+psk_vcycle\s*\(", txt)
    assert re.search(r"#define\s+PSK_VCYCLE_X0_GIVEN\s+1\b", txt)
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "psk_vcycle")
    res, args = N.SIGNATURES["psk_vcycle"]
    assert res is ctypes.c_int and len(args) == 8
    assert N.PSK_VCYCLE_X0_GIVEN == 1 and N.lib.psk_abi_version() == 4

"""The outer loop shared by svm.fit_squared_hinge and logreg.fit (clip_lite_amd/newton_cg.py), driven with stub callbacks and a CPU state
table that the stubs edit: the order of the calls, the CG loop lengths, where it ends and what it returns. Runs without a GPU or a simulator."""
import torch

from clip_lite_amd import hip, newton_cg


class _Stubs:
    """Callbacks that log their names. begin() plays newton_begin: at its k-th call it writes row k of `script` into the state table,
    one (active, cglast) pair per problem."""

    def __init__(self, script):
        self.script = script
        self.state = torch.zeros(len(script[0]), hip.SVM_STATE)
        self.state[:, hip.NCG_ACTIVE] = 1.0
        self.calls = []
        self.begins = 0

    def _log(self, name):
        return lambda: self.calls.append(name)

    def begin(self):
        self.calls.append("begin")
        row = self.script[min(self.begins, len(self.script) - 1)]
        for p, (active, cglast) in enumerate(row):
            self.state[p, hip.NCG_ACTIVE] = float(active)
            self.state[p, hip.NCG_CGLAST] = float(cglast)
        self.begins += 1

    def run(self, max_newton, max_cg, first_cap):
        return newton_cg.solve(self.state, self.begin, self._log("cg_update"), self._log("grad"), self._log("hess_vec"),
                               self._log("line_search"), max_newton, max_cg, first_cap)


def _iterations(calls):
    """Split the call log at every "grad"; check each iteration's order and return the CG loop lengths (None: ended after begin)."""
    caps, i = [], 0
    while i < len(calls):
        assert calls[i:i + 2] == ["grad", "begin"], calls[i:i + 2]
        i += 2
        if i == len(calls):
            caps.append(None)
            break
        cap = 0
        while calls[i:i + 2] == ["hess_vec", "cg_update"]:
            cap += 1
            i += 2
        assert calls[i] == "line_search", (i, calls[i])
        i += 1
        caps.append(cap)
    return caps


def test_call_order_caps_and_the_end():
    # three problems; problem 2 goes inactive at the second begin and carries the largest CGLAST from then on: it must not set a cap
    script = [
        [(1, 0), (1, 0), (1, 0)],            # first iteration: cap = first_cap
        [(1, 7), (1, 3), (0, 90)],           # 2 x 7 = 14
        [(1, 2), (1, 4), (0, 90)],           # 2 x 4 = 8 -> at least 10
        [(1, 30), (0, 99), (0, 90)],         # 2 x 30 = 60 -> at most max_cg = 40
        [(0, 5), (0, 99), (0, 90)],          # nothing active: the loop ends here
    ]
    s = _Stubs(script)
    launched = s.run(max_newton=30, max_cg=40, first_cap=6)
    caps = _iterations(s.calls)
    assert caps == [6, 14, 10, 40, None]
    assert s.calls[-2:] == ["grad", "begin"]                       # no line search after the read-back that found nothing active
    assert launched == 6 + 14 + 10 + 40
    assert s.calls.count("grad") == 5 and s.calls.count("line_search") == 4


def test_first_cap_is_taken_as_given():
    for first_cap in (3, 10, 100):
        s = _Stubs([[(1, 0)], [(0, 0)]])
        assert s.run(max_newton=5, max_cg=100, first_cap=first_cap) == first_cap
        assert _iterations(s.calls) == [first_cap, None]


def test_at_most_max_newton_plus_one_gradients():
    s = _Stubs([[(1, 1)]])                                          # a begin that never deactivates anything
    launched = s.run(max_newton=4, max_cg=25, first_cap=25)
    caps = _iterations(s.calls)
    assert s.calls.count("grad") == 5 == s.calls.count("begin")
    assert caps == [25, 10, 10, 10, 10] and launched == sum(caps)
    assert s.calls[-1] == "line_search"


def test_nothing_active_at_the_first_read_back():
    s = _Stubs([[(0, 0), (0, 0)]])
    assert s.run(max_newton=30, max_cg=100, first_cap=100) == 0
    assert s.calls == ["grad", "begin"]

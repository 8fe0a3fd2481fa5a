"""moved_search.choose, the rollout's choice among its neighbour searches (no
GPU, no engine): every combination of the flags against the control flow the
rollout's stage methods spelled out before the choice had one home, written
down again here; MovedMeshSearch.modes() and the engine's forwarding names."""
import inspect
import itertools

import pytest

from mmpde_amd import moved_search, ops
from mmpde_amd.moved_search import MovedMeshSearch, choose
from mmpde_amd.rollout import MMPDERollout

ROLES = ("graph", "query", "query1")


def _stages(radius_graph, knn_binned, radius_binned, N, have, use, burgers):
    """What the stage methods did, branch by branch.  have: the candidate
    tables exist (the graph's never with a radius graph); use: role -> the
    policy's use_table answer.  -> (mode per role, bins built, record computed)."""
    # _radius_binned()
    if not radius_graph:
        rb = False
    elif radius_binned is None:
        rb = bool(knn_binned) or N >= 9216
    else:
        rb = bool(radius_binned)
    # _st_main1
    bins = bool(knn_binned or rb)
    if knn_binned:
        use_g = use_q = False
        record = False
    else:
        use_g = (not radius_graph) and use["graph"]
        use_q = use["query"]
        record = have and (use_g or use_q)
    modes = {}
    # _st_main2, the graph (a *_moved call without a table is the full search)
    if radius_graph:
        modes["graph"] = "radius-binned" if rb else "radius"
    elif knn_binned:
        modes["graph"] = "binned"
    elif use_g:
        modes["graph"] = "table" if have else "full"
    else:
        modes["graph"] = "full"
    # _st_side2
    if knn_binned:
        modes["query"] = "binned"
    elif use_q:
        modes["query"] = "table" if have else "full"
    else:
        modes["query"] = "full"
    # _st_main2, Burgers' mode '1'
    if burgers:
        if knn_binned:
            modes["query1"] = "binned"
        elif use["query1"]:
            modes["query1"] = "table" if have else "full"
        else:
            modes["query1"] = "full"
    return modes, bins, bool(record)


def _cases():
    for radius, binned, rbin, N, have, burgers in itertools.product(
            (False, True), (False, True), (None, True, False), (2521, 4097, 9215, 9216), (True, False),
            (False, True)):
        roles = ROLES if burgers else ROLES[:2]
        for ans in itertools.product((True, False), repeat=len(roles)):
            yield radius, binned, rbin, N, have, burgers, dict(zip(roles, ans))


def _tables(radius, have, burgers):
    t = {"graph": have and not radius, "query": have}
    if burgers:
        t["query1"] = have
    return t


def test_radius_threshold_is_the_one_written_here():
    assert ops.RADIUS_BINNED_MIN_POINTS == 9216 and ops.KNN_BINNED_MIN_POINTS == 4097


def test_choose_every_combination():
    n = 0
    for radius, binned, rbin, N, have, burgers, use in _cases():
        want = _stages(radius, binned, rbin, N, have, use, burgers)
        got = choose(radius, binned, rbin, N, _tables(radius, have, burgers), use)
        assert (got.modes, got.bins, got.record) == want, (radius, binned, rbin, N, have, burgers, use)
        assert list(got.modes) == list(ROLES if burgers else ROLES[:2])
        n += 1
    assert n == 2 * 2 * 3 * 4 * 2 * (4 + 8)


@pytest.mark.parametrize("args, want", [
    # the 2521-point cylinder, tables answering: no bins, one record
    ((False, False, None, 2521, {"graph": True, "query": True}, {"graph": True, "query": True}),
     ({"graph": "table", "query": "table"}, False, True)),
    # the policy took the graph off its table: the record serves the query alone
    ((False, False, None, 2521, {"graph": True, "query": True}, {"graph": False, "query": True}),
     ({"graph": "full", "query": "table"}, False, True)),
    ((False, False, None, 2521, {"graph": True, "query": True}, {"graph": False, "query": False}),
     ({"graph": "full", "query": "full"}, False, False)),
    # 4500 points: no tables, everything through one binning
    ((False, True, None, 4500, {"graph": False, "query": False}, {}),
     ({"graph": "binned", "query": "binned"}, True, False)),
    ((True, True, None, 4500, {"graph": False, "query": False}, {}),
     ({"graph": "radius-binned", "query": "binned"}, True, False)),
    ((True, True, False, 4500, {"graph": False, "query": False}, {}),
     ({"graph": "radius", "query": "binned"}, True, False)),
    # Burgers 48 x 48 radius graph forced through bins built for it alone
    ((True, False, True, 2304, {"graph": False, "query": True, "query1": True},
      {"query": True, "query1": False}),
     ({"graph": "radius-binned", "query": "table", "query1": "full"}, True, True)),
    ((True, False, None, 9215, {"graph": False, "query": False}, {"query": True}),
     ({"graph": "radius", "query": "full"}, False, False)),
    ((True, False, None, 9216, {"graph": False, "query": False}, {"query": True}),
     ({"graph": "radius-binned", "query": "full"}, True, False)),
])
def test_choose_rows(args, want):
    got = choose(*args)
    assert (got.modes, got.bins, got.record) == want


class _Policy:
    def __init__(self, answers):
        self.state = dict.fromkeys(answers)
        self._a = answers

    def mode(self, role):
        return "table" if self._a[role] else "full"


def test_modes_agrees_with_choose():
    """modes() on an object holding only flags, table markers and a policy
    stand-in: the same answer as the choice, for every combination."""
    for radius, binned, rbin, N, have, burgers, use in _cases():
        s = MovedMeshSearch.__new__(MovedMeshSearch)
        s.radius_graph, s.knn_binned, s.radius_binned, s.N = radius, binned, rbin, N
        s.cand = {r: (object() if t else None) for r, t in _tables(radius, have, burgers).items()}
        s.policy = _Policy({r: a for r, a in use.items() if not (radius and r == "graph")})
        assert s.modes() == _stages(radius, binned, rbin, N, have, use, burgers)[0]


def test_engine_keeps_its_names():
    for name in ("knn_binned", "radius_binned"):
        p = inspect.getattr_static(MMPDERollout, name)
        assert isinstance(p, property) and p.fset is not None, name
    for name in ("knn_cand", "knn_cand_q"):
        assert isinstance(inspect.getattr_static(MMPDERollout, name), property), name
    for name in ("knn_modes", "knn_table_share", "knn_query_ties"):
        assert callable(getattr(MMPDERollout, name)), name
    src = inspect.getsource(MMPDERollout)
    for name in ("nbr_m", "deg_m", "idx1", "idx2"):
        assert f"self.{name}" in src, name
    # the choice and the searches live in one place
    assert "ops.knn_" not in src and "ops.radius_graph_nbr" not in src
    assert inspect.getsource(moved_search).count("def choose(") == 1

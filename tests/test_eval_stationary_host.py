"""Host tests of the stationary option of dp.EvalStep: the one staleness rule of the cached weight forms (_ops.form_stale) against
the expression each of its sites had written out before it existed, over every combination of (capturing, entry missing / derived
in this step / derived in an earlier step, version equal / moved, device equal / moved); what the stationary context changes in
that rule; the flag on the step."""
import itertools

import pytest
import torch


class _Form:
    """what the rule reads of a cached form: its device"""

    def __init__(self, device):
        self.device = device


DEV, OTHER = torch.device("cpu"), torch.device("meta")
VER, MOVED = (3, 4096, 7), (4, 4096, 7)


# the expression of each site as it stood, CTX.capturing -> cap, _ops.STEP_ID -> step; dev: the device the site compares with
def _rule_get(cap, ent, ver, dev, step):                  # Shadows.get, Shadows.stale
    return (cap and (ent is None or len(ent) < 3 or ent[2] != step)) or ent is None or ent[0] != ver or ent[1].device != dev


def _rule_cat(cap, ent, ver, dev, step):                  # Shadows.get_cat, get_cat_wb (weights and biases), _fp32._weight_split
    return (cap and (ent is None or ent[2] != step)) or ent is None or ent[0] != ver or ent[1].device != dev


def _rule_vec(cap, ent, ver, dev, step):                  # Shadows.get_cat_vec
    return (cap and (ent is None or ent[2] != step)) or ent is None or ent[0] != ver


def _rule_mx(cap, ent, ver, dev, step):                   # Shadows.get_cat_mx8, mx8_shadow
    return cap or ent is None or ent[0] != ver


def _rule_pad(cap, ent, ver, dev, step):                  # padded_shadow
    return cap or ent is None or ent[0] != ver or ent[1].device != dev


# site -> (its old expression, the arguments it gives form_stale: compares the device?, once per step?, entries carry a step id?)
SITES = {
    "Shadows.get": (_rule_get, True, True, True),
    "Shadows.stale": (_rule_get, True, True, True),
    "Shadows.get (entry without a step id)": (_rule_get, True, True, False),
    "Shadows.get_cat": (_rule_cat, True, True, True),
    "Shadows.get_cat_wb": (_rule_cat, True, True, True),
    "_fp32._weight_split": (_rule_cat, True, True, True),
    "Shadows.get_cat_vec": (_rule_vec, False, True, True),
    "Shadows.get_cat_mx8": (_rule_mx, False, False, False),
    "mx8_shadow": (_rule_mx, False, False, False),
    "padded_shadow": (_rule_pad, True, False, False),
}
STEP = 41
ENTRIES = ("missing", "this step", "earlier step")


def _entry(which, ver_moved, dev_moved, with_step):
    if which == "missing":
        return None
    ent = (MOVED if ver_moved else VER, _Form(OTHER if dev_moved else DEV))
    return ent + ((STEP if which == "this step" else STEP - 1),) if with_step else ent


@pytest.fixture()
def ops(monkeypatch):
    from hri_emo_amd import _ops
    ctx = _ops.StepContext()
    monkeypatch.setattr(_ops, "CTX", ctx)
    monkeypatch.setattr(_ops, "STEP_ID", STEP)
    return _ops


@pytest.mark.parametrize("site", list(SITES))
def test_the_rule_is_each_sites_old_expression(ops, site):
    old, with_dev, once, with_step = SITES[site]
    n = 0
    for cap, which, ver_moved, dev_moved in itertools.product((False, True), ENTRIES, (False, True), (False, True)):
        if not with_step and which == "earlier step":
            continue                  # such an entry says nothing about steps: one case for it
        ent = _entry(which, ver_moved, dev_moved, with_step)
        ops.CTX.capturing = cap
        got = ops.form_stale(ent, VER, DEV if with_dev else None, once_per_step=once)
        assert got == bool(old(cap, ent, VER, DEV, STEP)), (site, cap, which, ver_moved, dev_moved)
        n += 1
    assert n == (24 if with_step else 16)


@pytest.mark.parametrize("site", list(SITES))
def test_the_stationary_context_switches_the_rule_inside_a_capture_only(ops, site):
    old, with_dev, once, with_step = SITES[site]
    ops.CTX.stationary = True
    for cap, which, ver_moved, dev_moved in itertools.product((False, True), ENTRIES, (False, True), (False, True)):
        if not with_step and which == "earlier step":
            continue
        ent = _entry(which, ver_moved, dev_moved, with_step)
        ops.CTX.capturing = cap
        args = (ent, VER, DEV if with_dev else None)
        if not cap:                   # warm-up passes, eager forwards: the rule as it was
            assert ops.form_stale(*args, once_per_step=once) == bool(old(False, ent, VER, DEV, STEP))
            continue
        fresh = ent is not None and not ver_moved and not (with_dev and dev_moved)
        if fresh:                     # whatever step derived it: a stationary capture records no derivation
            assert ops.form_stale(*args, once_per_step=once) is False
        else:
            with pytest.raises(RuntimeError, match="stationary"):
                ops.form_stale(*args, once_per_step=once)


def test_no_site_spells_the_rule_out(ops):
    """the sites call form_stale: CTX.capturing is read by the rule's home alone among the cached weight forms"""
    import inspect
    from hri_emo_amd import _fp32
    S = ops.Shadows
    for fn in (S.get, S.stale, S.get_cat, S.get_cat_wb, S.get_cat_vec, S.get_cat_mx8, ops.padded_shadow, ops.mx8_shadow, _fp32._weight_split):
        src = inspect.getsource(fn)
        assert "form_stale(" in src and "CTX.capturing" not in src, fn.__qualname__


def test_the_form_log_keeps_a_pass_whole_and_a_known_key_once(ops):
    log = ops.FormLog()
    ops.CTX.forms = log
    f = lambda *a: None           # noqa: E731
    ops._note_form("a", f, 1)
    ops._note_form("a", f, 1)     # twice within one pass: the default capture pass asks twice as well
    ops._note_form("b", f, 2)
    assert [k for k, _, _ in log.take()] == ["a", "a", "b"]
    ops._note_form("a", f, 1)
    ops._note_form("c", f, 3)
    assert [k for k, _, _ in log.take()] == ["c"] and log.take() == []
    ops.CTX.forms = None
    ops._note_form("d", f, 4)
    assert log.new == [] and "d" not in log.known


def test_eval_step_stores_the_flag():
    import hri_emo_amd
    m = torch.nn.Linear(4, 4)
    assert hri_emo_amd.EvalStep(m).stationary is False
    assert hri_emo_amd.EvalStep(m, stationary=True).stationary is True
    assert hri_emo_amd.EvalStep(m, None, None, None, None, None, True).stationary is True
    ctx = hri_emo_amd.EvalStep(m, stationary=True).ctx
    assert ctx.stationary is False and ctx.forms is None and ctx.prologue is None, "the context is stationary inside a bucket pass only"

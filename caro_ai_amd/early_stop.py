"""Early stop of decided tau = 0 plies on the host: the rule's predicate in plain Python (what the kernels compute at the
root level of a descent; include/caro_hip.h, "early stop"), the argument check of SelfPlayEngine.set_early_stop, and the
counters self-play reports.

The rule itself runs in the engine (caro_engine_set_early_stop).  Nothing here needs a GPU."""
import numpy as np


def floor(min_minibatches):
    """min_minibatches as the engine takes it: an integer >= 1 (ValueError otherwise)"""
    m = min_minibatches
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) < 1:
        raise ValueError("early stop min_minibatches must be an integer >= 1, got %r" % (min_minibatches,))
    return int(m)


def decided(counts, m, budget, batch, min_minibatches=1):
    """The ply is decided at m: `counts` = the root's visit counts after m of the ply's minibatches have been backed up
    (None or empty: a root that is not in the tree, all zeros), budget = M, batch = B.  best = first maximum, n1 its
    count, n2 the largest count of the other actions (0 if there is none);
    min_minibatches <= m <= M - 2 and n1 - n2 > (M - m) * B."""
    if not min_minibatches <= m <= budget - 2:
        return False
    n = np.asarray(counts if counts is not None else [], dtype=np.int64).ravel()
    if n.size == 0:
        return False  # (0 - 0 > a positive number)
    best = int(np.argmax(n))  # first maximum
    n1 = int(n[best])
    rest = np.delete(n, best)
    n2 = int(rest.max()) if rest.size else 0
    return n1 - n2 > (budget - m) * batch


def ply_indices(games):
    """ply index of every tuple of a drain with the game records `games` ([n, 4]: a game has steps + 1 tuples, last ply
    first)"""
    counts = np.asarray(games).reshape(-1, 4)[:, 3].astype(np.int64) + 1
    return np.concatenate([np.arange(n - 1, -1, -1) for n in counts.tolist()]) if len(counts) else np.zeros(0, np.int64)


def stop_stats(drains, searches, steps_before_tau_0, fast=None, temperature=None):
    """What self-play reports over a list of drains (host arrays with "games", "mb" and, under the playout cap, "full"):
    stop_plies (plies that ran fewer minibatches than their budget), stop_tau0_plies (plies played at tau = 0, the ones
    the rule can cut) and stop_minibatches_saved (budget - minibatches run, summed).  A ply's budget is `searches`, or
    min(fast, searches) for a fast ply.  temperature: None or (tau_early, tau_late, visit_targets) of
    SelfPlayEngine.set_temperature -- a ply can be cut only if its move AND its tuple are at tau = 0 (include/caro_hip.h,
    "temperature"): none with visit targets, otherwise the early plies if tau_early is 0 and the late ones if tau_late is."""
    early0, late0 = False, True  # which plies are at tau = 0, move and tuple
    if temperature is not None:
        tau_e, tau_l, vt = temperature
        early0, late0 = (not vt) and tau_e == 0, (not vt) and tau_l == 0
    cut = tau0 = saved = 0
    for d in drains:
        mb = np.asarray(d["mb"]).astype(np.int64)
        budget = np.full(mb.shape, int(searches), np.int64)
        if fast is not None and "full" in d:
            budget[~np.asarray(d["full"]).astype(bool)] = min(int(fast), int(searches))
        idx = ply_indices(d["games"])
        assert idx.shape == mb.shape, (idx.shape, mb.shape)
        late = (idx >= steps_before_tau_0) | (steps_before_tau_0 <= 0)
        t0 = np.where(late, late0, early0)
        short = mb < budget
        cut += int(short.sum())
        tau0 += int(t0.sum())
        saved += int((budget - mb)[short].sum())
    return {"stop_plies": cut, "stop_tau0_plies": tau0, "stop_minibatches_saved": saved}

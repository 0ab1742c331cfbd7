"""The batched rule kernels (caro_rules_{legal,move,encode}_batch) at every geometry both board kinds allow: m,n,k and
caro, every n in 2..15 and every k in 2..n -- 210 (kind, n, k), all five V_M* and all five V_K* variants.  Each one
gets random playouts generated with the oracle's rules and the hand-built positions of tests/rules_cases.py (runs of
k - 1, k, k + 1 at every edge and corner in all four directions with open, half-blocked and blocked ends, overlines,
runs across the key's 64-bit word boundaries, a run of k elsewhere on a line through the move, full boards).  Next
key, won, board full, legal mask and planes must equal the oracle's on every transition."""
import numpy as np
import pytest
import torch

from tests.rules_cases import hand_built_cases
from tests.test_caro_cpu import _keys_of
from tests.test_gpu_engine import DEV, _game_of, _oracle_of

pytestmark = pytest.mark.gpu


def _random_playouts(o, n, rng, target):
    """whole random games on cell arrays until `target` transitions: (board before, move, player) each"""
    out = []
    while len(out) < target:
        b, p = np.full(n * n, 2, np.int8), int(rng.integers(2))
        while True:
            legal = o.possible_moves_cells(b)
            if not legal:
                break
            m = legal[int(rng.integers(len(legal)))]
            out.append((b, m, p))
            b2, won = o.move_cells(b, m, p)
            if won:
                break
            b, p = b2.astype(np.int8), 1 - p
    return out


def _check_geometry(kind, n, k, rng):
    from caro_ai_amd import _lib
    L = _lib.load()
    d = {"kind": kind, "n": n, "k": k}
    game, o = _game_of(d), _oracle_of(d)
    other = _oracle_of({"kind": "mnk" if kind == "caro" else "caro", "n": n, "k": k})
    hand = hand_built_cases(n, k)
    cases = hand + _random_playouts(o, n, rng, 600)
    M, A, HW, KW = len(cases), n * n, n * n, game.key_words
    before = np.stack([c[0] for c in cases]).astype(np.int8)
    mv = np.array([c[1] for c in cases], np.int32)
    pl = np.array([c[2] for c in cases], np.int32)
    after, won, full, legal, planes = [], [], [], [], []
    differ = blocked_draws = 0
    for i, (b, m, p) in enumerate(cases):
        a, w = o.move_cells(b, m, p)
        after.append(a)
        won.append(w)
        full.append(not o.possible_moves_cells(a))
        row = np.zeros(A, np.uint8)
        row[o.possible_moves_cells(b)] = 1
        legal.append(row)
        planes.append(o.planes_cells(a, 1 - p))
        if i < len(hand):
            w2 = other.move_cells(b, m, p)[1]
            differ += w != w2
            blocked_draws += full[-1] and not w and w2  # caro: a blocked k on the last empty cell
    after = np.stack(after).astype(np.int8)
    keys = torch.from_numpy(_keys_of(before.reshape(M, n, n), KW).view(np.int64)).to(DEV)
    moves = torch.from_numpy(mv).to(DEV)
    players = torch.from_numpy(pl).to(DEV)
    d_legal = torch.zeros((M, A), dtype=torch.uint8, device=DEV)
    _lib.check(L.caro_rules_legal_batch(game.kind, n, k, M, keys.data_ptr(), d_legal.data_ptr(), None))
    d_won = torch.zeros(M, dtype=torch.int32, device=DEV)
    d_full = torch.zeros(M, dtype=torch.int32, device=DEV)
    _lib.check(L.caro_rules_move_batch(game.kind, n, k, M, keys.data_ptr(), moves.data_ptr(), players.data_ptr(),
                                       d_won.data_ptr(), d_full.data_ptr(), None))
    who = (1 - players).contiguous()
    d_planes = torch.zeros((M, 2 * HW), dtype=torch.float32, device=DEV)
    _lib.check(L.caro_rules_encode_batch(game.kind, n, k, M, keys.data_ptr(), who.data_ptr(), d_planes.data_ptr(),
                                         None))
    torch.cuda.synchronize()
    got_keys = keys.cpu().numpy().view(np.uint64)
    want_keys = _keys_of(after.reshape(M, n, n), KW)
    bad = np.flatnonzero(~(got_keys == want_keys).all(1))
    assert bad.size == 0, ("key", kind, n, k, cases[bad[0]][0].tolist(), int(mv[bad[0]]), int(pl[bad[0]]))
    bad = np.flatnonzero(d_won.cpu().numpy().astype(bool) != np.array(won))
    assert bad.size == 0, ("won", kind, n, k, cases[bad[0]][0].tolist(), int(mv[bad[0]]), int(pl[bad[0]]), won[bad[0]])
    assert np.array_equal(d_full.cpu().numpy().astype(bool), np.array(full)), ("full", kind, n, k)
    assert np.array_equal(d_legal.cpu().numpy(), np.stack(legal)), ("legal", kind, n, k)
    assert np.array_equal(d_planes.cpu().numpy(), np.stack(planes)), ("planes", kind, n, k)
    return differ, blocked_draws, int(np.sum(won)), M


@pytest.mark.parametrize("kind", ["mnk", "caro"])
@pytest.mark.parametrize("n", range(2, 16))
def test_rules_kernels_vs_oracle_every_geometry(kind, n):
    rng = np.random.default_rng(31 * n + (kind == "caro"))
    for k in range(2, n + 1):
        differ, blocked_draws, wins, M = _check_geometry(kind, n, k, rng)
        assert wins > 0 and M > 600
        if n >= k + 2:  # room on a row for a run of k with an opponent stone at both ends: the two rules part
            assert differ > 0 and (kind == "mnk" or blocked_draws > 0), (kind, n, k, differ, blocked_draws)
        else:
            assert differ == 0, (kind, n, k)

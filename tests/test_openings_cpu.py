"""Random openings without a GPU (include/caro_hip.h, "openings"): the uniform against the construction written out
here, the host helper against the rule in plain Python on six games, the rule in Python against a version that uses
nothing but the C-ABI's single-state rule helpers, the distribution and the returned values, the argument checks, the
binding, and the train CLI's check."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from caro_ai_amd import _lib, openings
from caro_ai_amd.lib.game.caro import Caro
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.lib.game.tictactoe import TicTacToe
from tests.openings_ref import host_opening, kind_of

M64 = (1 << 64) - 1
SEED = 11
GAMES = [("c4", ConnectFour, (), 12), ("ttt3", TicTacToe, (3, 3), 8), ("mnk9", TicTacToe, (9, 5), 10),
         ("caro7", Caro, (7, 4), 10), ("mnk15", TicTacToe, (15, 5), 64), ("mnk4k2", TicTacToe, (4, 2), 6)]
N_UIDS = 2000


def _mix64(z):
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _open_uniform(seed, uid, i):
    """include/caro_noise.h, caro_open_uniform, written out: three splitmix64 rounds over the tag "open", the uid and
    the index, then the top 52 bits as a double strictly inside (0, 1)"""
    k = _mix64(seed ^ int.from_bytes(b"open", "big"))
    k = _mix64((k + uid) & M64)
    k = _mix64(k ^ i)
    return ((k >> 12) + 0.5) / 4503599627370496.0


def test_open_uniform_is_the_stated_construction_with_its_own_stream():
    L = _lib.load()
    rng = np.random.RandomState(1)
    same_cap = same_move = 0
    for _ in range(1000):
        seed = int(rng.randint(0, 2 ** 32)) << 32 | int(rng.randint(0, 2 ** 32))
        uid = int(rng.randint(0, 2 ** 32)) << int(rng.randint(0, 32))
        i = int(rng.randint(0, 66))
        u = L.caro_host_open_uniform(seed, uid, i)
        assert u == _open_uniform(seed, uid, i) == openings.open_uniform(seed, uid, i)
        assert 0.0 < u < 1.0
        same_cap += u == L.caro_host_cap_uniform(seed, uid, i)
        same_move += u == L.caro_host_move_uniform(seed, uid, i)
    assert same_cap == 0 and same_move == 0


def _opening_by_host_rules(game, seed, uid, first, max_plies):
    """the rule once more, with caro_host_initial / caro_host_legal / caro_host_move and the uniform written out above
    only; returns (key words, player, made, ended on the "not made" rule)"""
    L = _lib.load()
    kind, n, k = kind_of(game)
    KW, A = game.key_words, game.action_space
    key = (C.c_uint64 * KW)()
    assert L.caro_host_initial(kind, n, k, key) == 0
    legal = (C.c_uint8 * A)()
    player, made, refused = first, 0, False
    r = min(max_plies, int(_open_uniform(seed, uid, 0) * (max_plies + 1)))
    for i in range(r):
        assert L.caro_host_legal(kind, n, k, key, legal) == 0
        acts = [a for a in range(A) if legal[a]]
        a = acts[min(len(acts) - 1, int(_open_uniform(seed, uid, 1 + i) * len(acts)))]
        nxt = (C.c_uint64 * KW)(*key)
        won = C.c_int(0)
        assert L.caro_host_move(kind, n, k, nxt, a, player, C.byref(won)) == 0
        assert L.caro_host_legal(kind, n, k, nxt, legal) == 0
        if won.value or not any(legal):
            refused = True
            break
        key, player, made = nxt, 1 - player, made + 1
    return list(key), player, made, refused


@pytest.fixture(scope="module")
def opened():
    """{name: (game, max_plies, [(state, player, made) of openings.opening for uid 0 .. N_UIDS - 1])}, computed once"""
    out = {}
    for name, cls, args, mp in GAMES:
        game = cls(*args)
        out[name] = (game, mp, [openings.opening(game, SEED, uid, uid & 1, mp) for uid in range(N_UIDS)])
    return out


@pytest.mark.parametrize("name", [g[0] for g in GAMES])
def test_host_opening_equals_the_python_rule(opened, name):
    game, mp, want = opened[name]
    for uid, w in enumerate(want):
        assert host_opening(game, SEED, uid, uid & 1, mp) == w, uid


@pytest.mark.parametrize("name", ["ttt3", "mnk4k2", "c4"])
def test_python_rule_equals_the_rule_on_host_rule_helpers(opened, name):
    """... and in the two small games at least 1 % of the uids end on the "not made" rule"""
    game, mp, want = opened[name]
    refused = 0
    for uid, (state, player, made) in enumerate(want):
        key, p, m, ref = _opening_by_host_rules(game, SEED, uid, uid & 1, mp)
        assert (game.from_keys(np.array([key], dtype=np.uint64))[0], p, m) == (state, player, made), uid
        refused += ref
    print(name, "openings ended by a refused move:", refused, "of", N_UIDS)
    if name != "c4":
        assert refused >= N_UIDS // 100


@pytest.mark.parametrize("name", [g[0] for g in GAMES])
def test_distribution_and_returned_values(opened, name):
    game, mp, want = opened[name]
    rs = set()
    for uid, (state, player, made) in enumerate(want):
        r = min(mp, int(openings.open_uniform(SEED, uid, 0) * (mp + 1)))
        rs.add(r)
        assert 0 <= made <= r
        assert player == (uid & 1) ^ (made & 1)
        assert len(game.possible_moves(state)) > 0  # never full
        # never won: the position before the last opening ply was not won either, and that ply did not win -- replay it
        s, p = game.initial_state, uid & 1
        for i in range(made):
            legal = list(game.possible_moves(s))
            s, won = game.move(s, legal[min(len(legal) - 1, int(openings.open_uniform(SEED, uid, 1 + i) * len(legal)))], p)
            assert not won
            p = 1 - p
        assert s == state
    assert rs == set(range(mp + 1))
    for uid in range(50):
        assert openings.opening(game, SEED, uid, uid & 1, 0) == (game.initial_state, uid & 1, 0)
        assert host_opening(game, SEED, uid, uid & 1, 0) == (game.initial_state, uid & 1, 0)


def test_argument_checks_exports_and_the_drain_struct():
    L = _lib.load()
    key = (C.c_uint64 * 8)()
    p, m = C.c_int(), C.c_int()
    for kind, n, k, bad in [(0, 0, 0, -1), (0, 0, 0, 65), (0, 0, 0, 42), (1, 3, 3, 9), (1, 3, 3, -1), (1, 4, 2, 16),
                              (1, 15, 5, 65), (2, 7, 4, 49), (2, 7, 4, 50)]:
        assert L.caro_host_opening(kind, n, k, 1, 2, 0, bad, key, C.byref(p), C.byref(m)) == -22, (kind, n, bad)
        assert L.caro_openings_batch(kind, n, k, 1, bad, 1, None, None, None, None, None, None) == -22, (kind, n, bad)
    assert L.caro_host_opening(0, 0, 0, 1, 2, 2, 3, key, C.byref(p), C.byref(m)) == -22  # first must be 0 or 1
    assert L.caro_host_opening(1, 3, 3, 1, 2, 0, 8, key, C.byref(p), C.byref(m)) == 0
    assert L.caro_engine_set_openings(None, 4) == -22
    for name in ("caro_engine_set_openings", "caro_host_open_uniform", "caro_host_opening", "caro_openings_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.caro_version() >= 102
    for exc in (-1, 65, 9, True, 2.0):
        with pytest.raises(ValueError):
            openings.limit(exc, 9)
    assert openings.limit(8, 9) == 8 and openings.limit(0, 9) == 0 and openings.limit(12, 42) == 12
    # caro_drain_extra as include/caro_hip.h declares it (LP64: a uint32 size, then pointers) against the binding
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "caro_hip.h")).read()
    body = re.search(r"typedef struct caro_drain_extra \{(.*?)\} caro_drain_extra;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+)\s*(\*?)\s*(\w+);", body)
    assert [f[2] for f in fields] == ["size", "root_q_dev", "full_dev", "minibatches_dev", "open_dev"]
    assert fields[0][:2] == ("uint32_t", "") and all(f[1] == "*" for f in fields[1:]) and fields[4][0] == "int16_t"
    X = _lib.CaroDrainExtraOpen
    assert [f[0] for f in _lib.CaroDrainExtra._fields_ + X._fields_] == [f[2] for f in fields]
    assert [getattr(X, f[2]).offset for f in fields] == [0, 8, 16, 24, 32] and C.sizeof(X) == 40
    ex = X(None, None, None, 4096)
    assert ex.size == 40 and ex.open_dev == 4096 and not ex.minibatches_dev
    assert issubclass(X, _lib.CaroDrainExtra) and _lib.CaroDrainExtra().size == 32  # the shorter struct stays valid


def test_train_cli_refuses_bad_opening_plies():
    from caro_ai_amd import train
    for bad in ("-1", "65"):
        with pytest.raises(SystemExit) as e:
            train.main(["-g", "0", "-n", "t", "--opening-plies", bad])
        assert "--opening-plies N must be in [0, 64]" in str(e.value)
    args = train.parse_args(["-g", "0", "-n", "t", "--opening-plies", "4"])
    assert args.opening_plies == 4 and train.parse_args(["-g", "0", "-n", "t"]).opening_plies is None

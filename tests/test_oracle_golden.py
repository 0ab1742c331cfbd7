"""Pins the oracle (oracle/caro_oracle.c) against
  (a) the reference's own known-answer tests, restated as data, and
  (b) vectors recorded from the reference itself (tests/golden/make_golden.py).
CPU only.  These tests are what allows the GPU parity tests to trust the oracle.
"""
import hashlib
import os

import numpy as np
import pytest

from oracle.oracle import Oracle, noise_row
from tests.conftest import load_golden


def make_oracle(d, n_stores=1):
    if d["kind"] == "c4":
        return Oracle(Oracle.C4, n_stores=n_stores)
    return Oracle(Oracle.MNK, d["n"], d["k"], n_stores=n_stores)


# --------------------------------------------------------------- (a) known answers
class TestConnectFourKnownAnswers:
    """Values from lib/game/connect_four/test_connect_four.py:28-191."""

    EMPTY = 0b000000000000000000000000000000000000000000110110110110110110110
    FULL1 = 0b111111111111111111111111111111111111111111000000000000000000000

    def enc(self, o, cols):
        cells = np.full(42, 2, np.uint8)
        for c, col in enumerate(cols):
            for r, v in enumerate(col):
                cells[c * 6 + r] = v
        return o.to_int(cells)

    def dec(self, o, s):
        cells = o.to_cells(s)
        return [[int(cells[c * 6 + r]) for r in range(6) if cells[c * 6 + r] != 2] for c in range(7)]

    def test_encode_decode(self):
        o = Oracle(Oracle.C4)
        assert o.initial_state == self.EMPTY == 1797558
        assert self.enc(o, [[]] * 7) == self.EMPTY
        assert self.enc(o, [[1] * 6] * 7) == self.FULL1
        assert self.enc(o, [[0] * 6] * 7) == 0
        assert self.dec(o, self.EMPTY) == [[]] * 7
        assert self.dec(o, self.FULL1) == [[1] * 6] * 7
        assert self.dec(o, 0) == [[0] * 6] * 7

    def test_possible_moves(self):
        o = Oracle(Oracle.C4)
        assert o.possible_moves(0) == []
        assert o.possible_moves(self.FULL1) == []
        assert o.possible_moves(self.EMPTY) == [0, 1, 2, 3, 4, 5, 6]

    def test_vertical_win(self):
        o = Oracle(Oracle.C4)
        f = self.EMPTY
        for i, exp in enumerate([False, False, False, True]):
            f, won = o.move(f, 0, 1)
            assert won == exp
            assert self.dec(o, f) == [[1] * (i + 1)] + [[]] * 6

    def test_horizontal_win(self):
        o = Oracle(Oracle.C4)
        f = self.EMPTY
        for col, exp in [(0, False), (1, False), (3, False), (2, True)]:
            f, won = o.move(f, col, 1)
            assert won == exp
        assert self.dec(o, f) == [[1], [1], [1], [1], [], [], []]

    def test_diags(self):
        o = Oracle(Oracle.C4)
        f = self.enc(o, [[0, 0, 0, 1], [0, 0, 1], [0], [1], [], [], []])
        assert o.move(f, 2, 1)[1] is True
        assert o.move(f, 2, 0)[1] is False
        f = self.enc(o, [[], [0, 1], [0, 0, 1], [1, 0, 0, 1], [], [], []])
        assert o.move(f, 0, 1)[1] is True
        assert o.move(f, 0, 0)[1] is False

    def test_tricky(self):
        o = Oracle(Oracle.C4)
        f = self.enc(o, [[0, 1, 1], [1, 0], [0, 1], [0, 0, 1], [0, 0], [1, 1, 1, 0], []])
        s, won = o.move(f, 4, 0)
        assert won is True
        assert s == 3531389463375529686

    def test_model_view(self):
        o = Oracle(Oracle.C4)
        s = self.enc(o, [[0, 1, 0], [0], [1, 1, 1], [], [1], [], []])
        batch = o.states_to_training_batch([s, s], [1, 0])
        black_me = np.zeros((6, 7)); black_me[3, 2] = black_me[4, 0] = black_me[4, 2] = black_me[5, 2] = black_me[5, 4] = 1
        black_op = np.zeros((6, 7)); black_op[3, 0] = black_op[5, 0] = black_op[5, 1] = 1
        np.testing.assert_equal(batch[0], [black_me, black_op])
        np.testing.assert_equal(batch[1], [black_op, black_me])


class TestTicTacToeKnownAnswers:
    """Values from lib/game/tictactoe/test_tictactoe.py:12-144."""

    def test_codec(self):
        o = Oracle(Oracle.MNK, 3, 3)
        assert o.to_int([1, 2, 0, 0, 2, 0, 1, 0, 0]) == int("120020100")
        assert o.to_int([0, 0, 0, 1, 2, 0, 1, 0, 0]) == int("000120100")
        assert o.to_cells(int("010220011")).tolist() == [0, 1, 0, 2, 2, 0, 0, 1, 1]
        assert o.initial_state == 222222222

    def test_possible_moves(self):
        o = Oracle(Oracle.MNK, 3, 3)
        assert o.possible_moves(int("010220011")) == [3, 4]
        assert o.possible_moves(int("212220012")) == [0, 2, 3, 4, 8]

    def test_planes(self):
        o = Oracle(Oracle.MNK, 3, 3)
        b = o.states_to_training_batch([int("001010221"), int("101222001")], [1, 0])
        np.testing.assert_equal(b[0], [[[0, 0, 1], [0, 1, 0], [0, 0, 1]], [[1, 1, 0], [1, 0, 1], [0, 0, 0]]])
        np.testing.assert_equal(b[1], [[[0, 1, 0], [0, 0, 0], [1, 1, 0]], [[1, 0, 1], [0, 0, 0], [0, 0, 1]]])

    def test_moves(self):
        o = Oracle(Oracle.MNK, 3, 3)
        b = int("222222222")
        for mv, pl, exp in [(1, 0, "202222222"), (5, 1, "202221222"), (8, 0, "202221220"), (7, 1, "202221210")]:
            b, won = o.move(b, mv, pl)
            assert won is False and b == int(exp)

    @pytest.mark.parametrize("board,mv,pl,exp", [
        ("002112122", 2, 0, "000112122"), ("021012212", 6, 0, "021012012"),
        ("021102212", 8, 0, "021102210"), ("120122012", 4, 0, "120102012"),
        ("120102222", 6, 1, "120102122")])
    def test_winning_moves(self, board, mv, pl, exp):
        o = Oracle(Oracle.MNK, 3, 3)
        nb, won = o.move(int(board), mv, pl)
        assert won is True and nb == int(exp)


class TestBackupKnownAnswer:
    """lib/test_mcts.py:25-38: a 2-action mock game, states 1 -> 2 -> 3."""

    def test_back_up(self):
        o = Oracle(Oracle.MNK, 3, 3)  # any game; only A matters, we use 2 of the 9 slots
        A = o.A

        def pad(x, fill=0):
            return list(x) + [fill] * (A - len(x))

        keys = {1: np.full(9, 2, np.uint8), 2: np.full(9, 2, np.uint8), 3: np.full(9, 2, np.uint8)}
        keys[2][0] = 0
        keys[3][0] = 0; keys[3][1] = 1
        o.poke_node(keys[1], pad([0, 1]), pad([0.0, 0.5]), pad([0.0, 0.5]), pad([0.1, 0.9]))
        o.poke_node(keys[2], pad([1, 0]), pad([0.6, 0.0]), pad([0.6, 0.0]), pad([0.8, 0.2]))
        o.poke_node(keys[3], pad([0, 0]), pad([0.0, 0.0]), pad([0.0, 0.0]), pad([0.7, 0.3]))
        o.backup(0.2, np.stack([keys[1], keys[2], keys[3]]), [1, 0, 0])
        n1, n2, n3 = (o.get_node_cells(keys[i]) for i in (1, 2, 3))
        assert n1["N"][:2].tolist() == [0, 2] and n2["N"][:2].tolist() == [2, 0] and n3["N"][:2].tolist() == [1, 0]
        assert n1["W"][:2].tolist() == [0.0, 0.3] and n2["W"][:2].tolist() == [0.8, 0.0]
        assert n3["W"][:2].tolist() == [-0.2, 0.0]
        assert n1["Q"][:2].tolist() == [0.0, 0.15] and n2["Q"][:2].tolist() == [0.4, 0.0]
        assert n3["Q"][:2].tolist() == [-0.2, 0.0]


# --------------------------------------------------------------- (b) recorded from the reference
@pytest.mark.parametrize("name", ["rules_c4.json.gz", "rules_ttt3.json.gz", "rules_mnk5.json.gz",
                                  "rules_mnk15.json.gz"])
def test_rules_vs_reference(name):
    d = load_golden(name)
    o = make_oracle(d)
    assert len(d["recs"]) > 500
    for r in d["recs"]:
        s = int(r["s"])
        assert o.possible_moves(s) == r["legal"]
        s2, won = o.move(s, r["m"], r["p"])
        assert s2 == int(r["s2"]) and won == r["won"]
        planes = o.states_to_training_batch([s2], [1 - r["p"]])[0]
        assert np.packbits(planes.astype(np.uint8).reshape(-1)).tobytes().hex() == r["planes"]


def _check_game(o, g, net_setup):
    o.set_stream(g["seed"], g["uid"])
    if "noise_table" in g:  # explicit-table path
        o.set_noise_table(np.array(g["noise_table"]))
        o.set_uniform_table(np.array(g["uniform_table"]))
    else:
        o.set_noise_table(None)
        o.set_uniform_table(None)
    net_setup(o)
    res = o.play_game(g["steps_before_tau_0"], g["searches"], g["batch"], g["first_player"])
    assert res["result"] == g["result"]
    assert res["steps"] == g["steps"]
    assert res["plies"] == g["plies"]
    assert [str(s) for s in res["states"]] == g["states"]
    assert res["players"].tolist() == g["players"]
    assert res["z"].tolist() == g["z"]
    for ply in range(g["plies"]):
        assert res["rootN"][ply].tolist() == g["trace"][ply]["N"], ply
        assert res["nodes"][ply] == g["trace"][ply]["nodes"], ply
        assert res["pi"][ply].tolist() == g["pi"][ply], ply  # float64, bit exact
    return res


@pytest.mark.parametrize("name", ["synth_c4.json.gz", "synth_ttt3.json.gz", "synth_mnk5.json.gz",
                                  "synth_mnk15.json.gz"])
def test_search_vs_reference_synth_net(name):
    """G2: select / dedupe / expand / backup / policy / play_game with the
    synthetic table net: every integer and every float64 pi bit exact."""
    d = load_golden(name)
    for g in d["games"]:
        o = make_oracle(d, g["n_stores"])
        _check_game(o, g, lambda oo: oo.use_synth_net())


def test_noise_spec_matches_recorded_tables():
    d = load_golden("synth_c4.json.gz")
    g = d["games"][0]
    tab = np.array(g["noise_table"])
    assert hashlib.sha1(tab.tobytes()).hexdigest() == g["noise_sha1"]
    # first row is (ply 0, sim 8): the root is expanded by the first minibatch (Q6)
    np.testing.assert_array_equal(tab[0], noise_row(g["seed"], g["uid"], 0, 8, 7))
    assert abs(tab.sum(axis=1) - 1).max() < 1e-12
    assert tab.min() > 0


def test_root_WQ_dtypes_vs_reference():
    """W / Q values and their NEP-50 dtype (python float vs float32) at the
    root after every ply's search."""
    d = load_golden("synth_c4.json.gz")
    g = d["games"][1]
    o = make_oracle(d, g["n_stores"])
    o.use_synth_net()
    o.set_stream(g["seed"], g["uid"])
    # replay the game ply by ply with search_batch so the tree can be inspected
    state = o.initial_state
    player = g["first_player"]
    for ply in range(g["plies"]):
        assert str(state) == g["states"][ply]
        o.search_batch(g["searches"], g["batch"], state, player, ply=ply)
        nd = o.get_node(state)
        tr = g["trace"][ply]
        assert nd["N"].tolist() == tr["N"]
        assert nd["W"].tolist() == tr["W"]
        assert nd["Q"].tolist() == tr["Q"]
        assert nd["W_is_f32"].tolist() == tr["W_f32"]
        pi = np.array(g["pi"][ply])
        nxt = [i for i in range(o.A)]
        # the move actually played: recover from the next recorded state
        if ply + 1 < g["plies"]:
            for a in o.possible_moves(state):
                s2, _ = o.move(state, a, player)
                if str(s2) == g["states"][ply + 1]:
                    state = s2
                    break
            else:
                raise AssertionError("no move leads to the recorded next state")
            player = 1 - player
        del pi, nxt


# --------------------------------------------------------------- real weights (G3 / G5)
def _torch_net(path, shape, A):
    import os
    import torch
    from caro_ai_amd.lib.model import Net
    from tests.conftest import GOLDEN
    torch.set_num_threads(1)
    net = Net(shape, A)
    net.load_state_dict(torch.load(os.path.join(GOLDEN, "weights", path), map_location="cpu"))
    net.eval()

    def fn(planes, states, players):
        with torch.no_grad():
            logits, values = net(torch.from_numpy(np.ascontiguousarray(planes)))
            return torch.softmax(logits, dim=1).numpy(), values.numpy()[:, 0]

    return fn


@pytest.mark.parametrize("name", ["real_c4.json.gz", "real_ttt3.json.gz", "arena_c4.json.gz"])
def test_play_game_vs_reference_real_weights(name):
    """G3 / G5: the oracle driving the SAME torch CPU float32 forward on the
    same leaf batches reproduces the reference's games exactly (the net is
    third-party arithmetic; identical batches give identical bits)."""
    d = load_golden(name)
    w = d["weights"] if isinstance(d["weights"], list) else [d["weights"], d["weights"]]
    for g in d["games"]:
        o = make_oracle(d, g["n_stores"])
        shape = (2, o.rows, o.cols)

        def setup(oo):
            oo.set_net(0, _torch_net(w[0], shape, oo.A))
            oo.set_net(1, _torch_net(w[1], shape, oo.A))

        _check_game(o, g, setup)


# --------------------------------------------------------------- round 3: BASELINE config 4 at its real size
def seeded_net_15(seed):
    """the 15 x 15 net is this repo's own `Net` under torch.manual_seed(seed) -- the seed is what
    tests/golden/make_golden_r3.py committed; it loaded the resulting state_dict into the reference's Net."""
    import torch
    from caro_ai_amd.lib.model import Net
    torch.manual_seed(seed)
    return Net((2, 15, 15), 225).eval()


def state_dict_sha256(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_config4_table_net_games_400_sims():
    """G2 at config 4's per-game settings: TicTacToe(15, 5), 50 x 8 sims/move, tau = 1 for 10 plies; the
    reference's whole games (65-75 plies, thousands of nodes) -- root N / node count / pi / z bit exact"""
    d = load_golden("synth_mnk15_400.json.gz")
    assert len(d["games"]) >= 2
    for g in d["games"]:
        assert (g["searches"], g["batch"]) == (50, 8) and g["plies"] > 30
        o = make_oracle(d, g["n_stores"])
        _check_game(o, g, lambda oo: oo.use_synth_net())


def test_config4_conv_net_games_400_sims():
    """G3 for 15 x 15: seeded own-Net weights (the fixture's SHA-256 says they are the recorded ones), the
    reference's games at 50 x 8 against the oracle driving the same torch CPU forward"""
    import torch
    d = load_golden("real_mnk15.json.gz")
    net = seeded_net_15(d["weights_seed"])
    assert state_dict_sha256(net.state_dict()) == d["weights_sha256"]
    torch.set_num_threads(1)

    def fn(planes, states, players):
        with torch.no_grad():
            logits, values = net(torch.from_numpy(np.ascontiguousarray(planes)))
            return torch.softmax(logits, dim=1).numpy(), values.numpy()[:, 0]

    for g in d["games"][:2]:  # ~10 s each on one core; the GPU tests use all of them
        o = make_oracle(d, g["n_stores"])

        def setup(oo):
            oo.set_net(0, fn)
            oo.set_net(1, fn)

        _check_game(o, g, setup)


# --------------------------------------------------------------- persistent stores (make_golden_r4.py)
def _replay_on_persistent_stores(o, games, sbt0, searches, batch, two_stores):
    """The reference's play_game loop (lib/utils.py:63-99) driven step by step on stores that are NOT cleared between
    games -- train.py:184-193's shared self-play store, train.py:134-141's pair of evaluate stores -- with the
    recorded root N / W / Q (+ float32 flags) and len(store) checked after every search_batch."""
    from oracle.oracle import move_uniform, sample_index
    for gm in games:
        o.set_stream(gm["seed"], gm["uid"])
        state, player, step = o.initial_state, gm["first_player"], 0
        result = None
        for ply, tr in enumerate(gm["trace"]):
            assert (str(state), player) == (tr["state"], tr["player"]), (gm["uid"], ply)
            st = player if two_stores else 0
            o.search_batch(searches, batch, state, player, store=st, which_net=player if two_stores else 0, ply=ply)
            nd = o.get_node(state, store=st)
            assert nd["N"].tolist() == tr["N"], (gm["uid"], ply)
            assert nd["W"].tolist() == tr["W"] and nd["W_is_f32"].tolist() == tr["W_f32"], (gm["uid"], ply)
            assert nd["Q"].tolist() == tr["Q"], (gm["uid"], ply)
            assert o.store_len(st) == tr["nodes"], (gm["uid"], ply)
            tau = 1 if step < sbt0 else 0
            a = sample_index(o.get_policy(state, tau, store=st), move_uniform(gm["seed"], gm["uid"], ply))
            state, won = o.move(state, a, player)
            if won:
                result = 1 if player == 0 else -1
                break
            player = 1 - player
            if not o.possible_moves(state):
                result = 0
                break
            step += 1
        assert ply == gm["plies"] - 1 and (result, step) == (gm["result"], gm["steps"]), gm["uid"]
        lens = [o.store_len(s) for s in range(2 if two_stores else 1)]
        assert lens == (gm["store_len_after"] if two_stores else [gm["store_len_after"]])


def test_shared_self_play_store_across_games_vs_reference():
    """ref train.py:184-193 + :41-47: ONE MCTS for every self-play game -- the second and third game search on the
    statistics the earlier ones left (the root is expanded from the first minibatch on, so even the number of
    Dirichlet rows differs from a fresh store's)"""
    d = load_golden("persist_selfplay_c4.json.gz")
    o = make_oracle(d, 1)
    o.use_synth_net(*d["salts"])
    _replay_on_persistent_stores(o, d["games"], d["steps_before_tau_0"], d["searches"], d["batch"], False)
    assert d["games"][1]["trace"][0]["nodes"] > d["games"][0]["store_len_after"] - 1  # game 2 started on a full store


def test_evaluate_pair_of_stores_across_rounds_vs_reference():
    """ref train.py:134-141: the pair [MCTS, MCTS] is built once and reused by all rounds (20 x 16 sims, tau = 0)"""
    d = load_golden("persist_evaluate_c4.json.gz")
    o = make_oracle(d, 2)
    o.use_synth_net(*d["salts"])
    _replay_on_persistent_stores(o, d["rounds"], d["steps_before_tau_0"], d["searches"], d["batch"], True)
    res = [g["result"] for g in d["rounds"]]
    assert d["win_ratio"] == res.count(1) / len(res)


# --------------------------------------------------------------- round 5: draws, G1 at SURVEY's size, G5 (make_golden_r5.py)
def test_drawn_games_vs_reference():
    """ref lib/utils.py:86-96 (no legal move left => result 0, every z 0) and lib/mcts.py:144-146 (a full board met
    inside the tree backs up 0.0): whole TicTacToe(3,3) games recorded from the reference that END IN A DRAW -- 25x1,
    10x8, 25x4 on one store, 10x8 and 20x16 on one store per player -- root N / nodes / pi / z bit exact"""
    d = load_golden("draws_ttt3.json.gz")
    assert len(d["games"]) >= 3
    shapes = set()
    for g in d["games"]:
        assert g["result"] == 0 and g["plies"] == 9 and g["steps"] == 8 and set(g["z"]) == {0}
        shapes.add((g["searches"], g["batch"], g["n_stores"]))
        o = make_oracle(d, g["n_stores"])
        res = _check_game(o, g, lambda oo: oo.use_synth_net())
        assert res["result"] == 0 and not res["z"].any()
    assert len(shapes) >= 3 and any(s[2] == 2 for s in shapes)


@pytest.mark.parametrize("name", ["c4", "ttt3", "mnk15", "mnk5", "mnk8", "mnk10"])
def test_rules_digest_vs_reference(name):
    """SURVEY 8(c) G1 at its stated size -- 10^5 random connect-four plies, 10^4 each for 3x3 and 15x15 k=5, played
    through the reference's game classes and kept as one SHA-256 per 1000-ply block over (next state, won, legal mask,
    planes): the oracle walks the same blocks and must produce the same digests"""
    from tests import rules_digest as rd
    d = load_golden("rules_digest.json.gz")
    s = d["sets"][name]
    o = make_oracle(s)
    assert len(s["blocks"]) * d["block"] == {"c4": 100000, "ttt3": 10000, "mnk15": 10000}.get(name, 5000)
    for b, want in enumerate(s["blocks"]):
        assert rd.block_digest(o, d["seed"], b, d["block"], o.A) == want, (name, b)


@pytest.mark.parametrize("name", ["arena_c4_320_x16.json.gz", "arena_c4_800_x16.json.gz"])
def test_arena_32_games_vs_reference(name):
    """32 seeded tau = 0 arena games best_026 vs best_025, one store per player, recorded from the
    reference -- 16 at play.py's 40 x 8 sims/move (ref play.py:47-52, config.py:18-19), 16 at BASELINE config 5's
    100 x 8: the oracle driving the same torch CPU forward reproduces every ply's root N (= the argmax move), pi, z,
    and the W / L / D tally"""
    d = load_golden(name)
    assert len(d["games"]) == 16
    res = []
    nets = None
    # under the CPU sanitizers (oracle/asan/run.sh; tests/test_sanitizers.py) the first two games of each set keep the
    # two-store / two-net paths of the oracle instrumented without the minutes all 32 take there
    games = d["games"][:2] if os.environ.get("CARO_UNDER_ASAN") else d["games"]
    for g in games:
        assert g["steps_before_tau_0"] == 0 and g["n_stores"] == 2 and g["first_player"] == g["uid"] & 1
        o = make_oracle(d, 2)
        if nets is None:
            nets = [_torch_net(w, (2, o.rows, o.cols), o.A) for w in d["weights"]]

        def setup(oo):
            oo.set_net(0, nets[0])
            oo.set_net(1, nets[1])

        r = _check_game(o, g, setup)
        for ply in range(g["plies"]):  # tau = 0: pi is the one-hot of the first maximum of N
            n = g["trace"][ply]["N"]
            assert g["pi"][ply].index(1.0) == n.index(max(n)) and sum(g["pi"][ply]) == 1.0
        res.append(r["result"])
    if len(games) == 16:
        assert {"wins": res.count(1), "losses": res.count(-1), "draws": res.count(0)} == d["tally"]


def test_reference_callers_themselves_produce_the_round4_fixtures():
    """the persistent-store fixtures of round 4 were recorded by calling the reference's `play_game` in a hand-written
    copy of the call pattern of `self_play` / `evaluate`.  tests/golden/make_golden_r5_callers.py ran the reference's
    OWN `train.self_play` (ref train.py:24-59) and `train.evaluate` (:120-149) under the same harness and asserted, ply
    by ply, that they produce exactly those fixtures; what it wrote down is compared here with the fixtures the oracle
    (above) and the GPU shim (tests/test_gpu_shim.py) reproduce bit for bit: the drop-in callers are pinned to the real
    functions, not to a reading of them."""
    chk = load_golden("callers_check.json.gz")
    sp = load_golden("persist_selfplay_c4.json.gz")
    ev = load_golden("persist_evaluate_c4.json.gz")
    assert [(c["uid"], c["result"], c["steps"], c["store_len_after"]) for c in chk["self_play"]["calls"]] == \
        [(g["uid"], g["result"], g["steps"], g["store_len_after"]) for g in sp["games"]]
    for c, g in zip(chk["self_play"]["calls"], sp["games"]):
        h = hashlib.sha256()
        r = g["replay"]
        for s, p, pi, z in zip(r["states"], r["players"], r["pi"], r["z"]):
            h.update(("%d|%d|%s|%d;" % (int(s), int(p), ",".join(repr(float(x)) for x in pi), int(z))).encode())
        assert h.hexdigest() == c["replay_sha256"] and len(r["z"]) == c["replay_rows"]
    assert chk["self_play"]["tracked"] == ["speed_nodes", "speed_steps"]   # the metric names train.py:53-54 reports
    assert [(c["uid"], c["result"], c["steps"]) for c in chk["evaluate"]["rounds"]] == \
        [(g["uid"], g["result"], g["steps"]) for g in ev["rounds"]]
    assert chk["evaluate"]["win_ratio"] == ev["win_ratio"]


def test_mid_size_boards_whole_games_vs_reference():
    """whole table-net games recorded from the reference on 6x6 k4, 8x8 k5 (one store, and one per player) and 10x10 k5
    (tests/golden/make_golden_r5.py mid): the lane geometries between 5x5 and 15x15 -- root N / nodes / pi / z bit exact"""
    d = load_golden("synth_mid.json.gz")
    assert {(g["n"], g["k"]) for g in d["games"]} == {(6, 4), (8, 5), (10, 5)}
    for g in d["games"]:
        o = Oracle(Oracle.MNK, g["n"], g["k"], n_stores=g["n_stores"])
        _check_game(o, g, lambda oo: oo.use_synth_net())


# --------------------------------------------------------------- caro (kind 2): the blocked-k rule of include/caro_hip.h
# The reference has no caro; its vectors were recorded from the reference's search driven by a plain-Python statement
# of the rule (tests/golden/make_golden_caro.py).  The oracle's caro win test walks the lines cell by cell and shares
# no code with the bit forms in caro_rules.h.
def _random_boards(n, M, rng):
    """M random boards (fill 10-95 %), each with a random empty cell and a random mover"""
    fill = rng.uniform(0.1, 0.95, M)
    boards = np.where(rng.random((M, n * n)) < fill[:, None], rng.integers(0, 2, (M, n * n)), 2).astype(np.int8)
    out = []
    for i in range(M):
        empty = np.flatnonzero(boards[i] == 2)
        if empty.size == 0:
            boards[i, rng.integers(n * n)] = 2
            empty = np.flatnonzero(boards[i] == 2)
        out.append((boards[i], int(empty[rng.integers(empty.size)]), int(rng.integers(2))))
    return out


def test_caro_rules_vs_reference_recorded_transitions():
    """every rules_caro transition: the oracle's caro move gives the recorded next state and caro result, its m,n,k
    move on the same transition the recorded gomoku result"""
    d = load_golden("rules_caro.json.gz")
    assert d["kind"] == "caro"
    differ = total = 0
    for b in d["boards"]:
        o, t = Oracle(Oracle.CARO, b["n"], b["k"]), Oracle(Oracle.MNK, b["n"], b["k"])
        for r in b["recs"]:
            s = int(r["s"])
            assert o.possible_moves(s) == t.possible_moves(s)
            assert o.move(s, r["m"], r["p"]) == (int(r["s2"]), r["caro"]), (b["n"], r)
            assert t.move(s, r["m"], r["p"]) == (int(r["s2"]), r["gomoku"]), (b["n"], r)
            differ += r["caro"] != r["gomoku"]
            total += 1
    assert total == 1340 and differ >= 200


def test_caro_search_vs_reference_synth_net():
    """every synth_caro game, the 50 x 8 one on 15 x 15 included, replayed by the oracle with the table net: root N,
    node counts, every integer and every float64 pi bit exact"""
    d = load_golden("synth_caro.json.gz")
    assert any(g["searches"] == 50 for g in d["games"])
    games = d["games"]
    if os.environ.get("CARO_UNDER_ASAN"):
        games = [g for g in games if g["searches"] != 50][:4]
    for g in games:
        o = Oracle(Oracle.CARO, g["n"], g["k"], n_stores=g["n_stores"])
        _check_game(o, g, lambda oo: oo.use_synth_net())


@pytest.mark.parametrize("n", range(2, 16))
def test_caro_move_vs_numpy_restatement_every_k(n):
    """for every k in 2..n: random positions and the hand-built ones (tests/rules_cases.py: runs of k - 1, k, k + 1 at
    every edge and corner, blocked / half-blocked / open ends, runs elsewhere on the line, word boundaries, full
    boards) -- the oracle's caro won flag against tests/test_caro_cpu.py's numpy restatement of the rule, and the
    next board against the board with the stone placed"""
    from tests.rules_cases import hand_built_cases
    from tests.test_caro_cpu import numpy_caro_won
    rng = np.random.default_rng(n)
    for k in range(2, n + 1):
        o, t = Oracle(Oracle.CARO, n, k), Oracle(Oracle.MNK, n, k)
        cases = hand_built_cases(n, k) + _random_boards(n, 150, rng)
        wins = differ = 0
        for board, mv, p in cases:
            after, won = o.move_cells(board, mv, p)
            want = board.copy()
            want[mv] = p
            assert np.array_equal(after, want)
            r, c = divmod(mv, n)
            assert won == numpy_caro_won(want.reshape(n, n), r, c, k, p), (n, k, board.tolist(), mv, p)
            wins += won
            differ += won != t.move_cells(board, mv, p)[1]
        assert wins >= 4, (n, k)  # hand-built open runs of k at least
        if n >= k + 2:  # a line with room for an opponent stone at both ends of a run of k: the rules differ
            assert differ > 0, (n, k)
        else:
            assert differ == 0, (n, k)


@pytest.mark.parametrize("n", range(2, 16))
def test_caro_with_k_equal_n_is_mnk(n):
    """Oracle(CARO, n, n) and Oracle(MNK, n, n) on random playouts: legal moves, next state, won flag and planes"""
    o, t = Oracle(Oracle.CARO, n, n), Oracle(Oracle.MNK, n, n)
    rng = np.random.default_rng(100 + n)
    plies = 0
    for _ in range(60 if n <= 6 else 12):
        s, p = o.initial_state, int(rng.integers(2))
        while True:
            legal = o.possible_moves(s)
            assert legal == t.possible_moves(s)
            if not legal:
                break
            mv = legal[int(rng.integers(len(legal)))]
            a, b = o.move(s, mv, p), t.move(s, mv, p)
            assert a == b
            assert np.array_equal(o.states_to_training_batch([a[0]], [1 - p]), t.states_to_training_batch([a[0]], [1 - p]))
            plies += 1
            s, p = a[0], 1 - p
            if a[1]:
                break
    assert plies > 100

"""Paired openings for arena matches, without a GPU: the rule in plain Python (caro_ai_amd.openings.opening with
paired=True), the twin property of the two games of a pair, and the refusals of play_games, evaluate and the two CLIs,
all raised before an engine is built."""
import numpy as np
import pytest

from caro_ai_amd import openings
from caro_ai_amd.lib.game.caro import Caro
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.lib.game.tictactoe import TicTacToe
from tests.openings_ref import host_opening

SEED, MAX_PLIES = 5, 6
GAMES = {"c4": lambda: ConnectFour(), "mnk5": lambda: TicTacToe(5, 4), "caro7": lambda: Caro(7, 4)}


def test_pair_key_and_paired_rule_are_the_rule_at_uid_shifted():
    game = ConnectFour()
    assert [openings.pair_key(u) for u in (0, 1, 2, 3, 7100, 7101, (1 << 40) + 1)] == [0, 0, 1, 1, 3550, 3550, 1 << 39]
    for uid in list(range(16)) + [7100, 7101, (1 << 40) + 5]:
        for first in (0, 1):
            want = openings.opening(game, SEED, uid >> 1, first, MAX_PLIES)
            assert openings.opening(game, SEED, uid, first, MAX_PLIES, paired=True) == want
            assert host_opening(game, SEED, uid >> 1, first, MAX_PLIES) == want  # (the C-ABI helper takes the key)
            assert openings.opening(game, SEED, uid, first, MAX_PLIES, paired=False) == \
                openings.opening(game, SEED, uid, first, MAX_PLIES)


def test_drawn_lengths_of_the_first_eight_pairs():
    """the sample holds zero, odd and even lengths (computed from open_uniform)"""
    r = [min(MAX_PLIES, int(openings.open_uniform(SEED, key, 0) * (MAX_PLIES + 1))) for key in range(8)]
    assert r == [2, 3, 0, 4, 4, 2, 0, 6]


@pytest.mark.parametrize("name", list(GAMES))
def test_the_two_games_of_a_pair_are_colour_swapped_twins(name):
    """games 2j and 2j + 1 (first player = uid & 1): the same number of opening plies, opposite movers, and the same
    planes when each is encoded for its own mover -- the same stones with the players exchanged"""
    game = GAMES[name]()
    made_all = []
    for j in range(8):
        s0, p0, m0 = openings.opening(game, SEED, 2 * j, 0, MAX_PLIES, paired=True)
        s1, p1, m1 = openings.opening(game, SEED, 2 * j + 1, 1, MAX_PLIES, paired=True)
        assert m0 == m1 and p0 == 1 - p1 and p0 == (m0 & 1)
        planes = game.states_to_training_batch([s0, s1], [p0, p1])  # caro_host_encode, each for its own mover
        assert planes.dtype == np.float32 and np.array_equal(planes[0], planes[1])
        assert int(planes[0].sum()) == m0 and (s0 == s1) == (m0 == 0)
        # seen by ONE player the twins differ as soon as a stone is on the board
        one = game.states_to_training_batch([s0, s1], [0, 0])
        assert np.array_equal(one[0], one[1]) == (m0 == 0)
        made_all.append(m0)
    assert any(m & 1 for m in made_all) and any(m == 0 for m in made_all), made_all
    # without the pairing the two games open differently somewhere in the sample
    assert any(openings.opening(game, SEED, 2 * j, 0, MAX_PLIES)[2] != openings.opening(game, SEED, 2 * j + 1, 1, MAX_PLIES)[2]
               for j in range(8))


def test_play_games_refuses_bad_pair_arguments_before_an_engine_is_built():
    from caro_ai_amd.lib.utils import play_games
    game, a, b = ConnectFour(), object(), object()
    for kw, word in ((dict(openings=None), "openings"), (dict(openings=0), "openings"),
                     (dict(openings=4, first_player_mode=0), "first_player_mode"),
                     (dict(openings=4, uid_base=7), "uid_base"), (dict(openings=4, n_games=5), "n_games")):
        args = dict(n_games=4, openings=4)
        args.update(kw)
        n = args.pop("n_games")
        with pytest.raises(ValueError, match="opening_pairs.*" + word):
            play_games(game, n, None, a, b, opening_pairs=True, **args)
    with pytest.raises(ValueError, match="opening plies"):
        play_games(game, 4, None, a, b, openings=42, opening_pairs=True)
    # an arena opens in pairs or not at all
    with pytest.raises(ValueError, match="only in pairs"):
        play_games(game, 4, None, a, b, openings=4)
    # the other arena refusals stay word for word
    for kw, text in ((dict(resign=(-0.9, 0.1)), "play_games: arena games never resign"),
                     (dict(playout_cap=(0.5, 2)), "play_games: arena games never use the playout cap"),
                     (dict(early_stop=1), "play_games: arena games never stop a ply early"),
                     (dict(forced_playouts=2.0), "play_games: arena games never use forced playouts")):
        with pytest.raises(ValueError) as e:
            play_games(game, 4, None, a, b, **kw)
        assert str(e.value) == text


def test_evaluate_and_fit_refuse_bad_opening_arguments_before_an_engine_is_built():
    from caro_ai_amd import train
    game, a, b = ConnectFour(), object(), object()
    with pytest.raises(ValueError, match="rounds must be even"):
        train.evaluate(game, a, b, rounds=7, opening_plies=4)
    with pytest.raises(ValueError, match="reference_stores"):
        train.evaluate(game, a, b, rounds=8, opening_plies=4, reference_stores=True)
    with pytest.raises(ValueError, match="opening plies"):
        train.evaluate(game, a, b, rounds=8, opening_plies=42)
    with pytest.raises(ValueError, match="reference_evaluate"):
        train.fit(game, None, "cpu", 4, eval_opening_plies=4, reference_evaluate=True)


def test_train_cli_checks_eval_opening_plies():
    from caro_ai_amd import train
    game = ConnectFour()

    def parsed(*extra):
        return train.parse_args(["-n", "r", "-g", "0", "--cuda"] + list(extra))

    assert train.eval_openings_from_args(parsed(), game) is None
    assert train.eval_openings_from_args(parsed("--eval-opening-plies", "0"), game) is None
    assert train.eval_openings_from_args(parsed("--eval-opening-plies", "4"), game) == 4
    assert parsed("--eval-opening-plies", "4").opening_plies is None  # (self-play's own flag is another one)
    with pytest.raises(SystemExit, match="--reference-evaluate"):
        train.eval_openings_from_args(parsed("--eval-opening-plies", "4", "--reference-evaluate"), game)
    for bad in ("42", "-1", "65"):
        with pytest.raises(SystemExit, match="--eval-opening-plies N must be"):
            train.eval_openings_from_args(parsed("--eval-opening-plies", bad), game)
    with pytest.raises(SystemExit, match="--reference-evaluate"):  # (main refuses before it touches a device)
        train.main(["-n", "r", "-g", "0", "--cuda", "--eval-opening-plies", "4", "--reference-evaluate"])


def test_play_cli_checks_opening_plies(capsys):
    from caro_ai_amd import play
    base = ["-g", "0", "--cuda", "a.dat", "b.dat"]
    assert play.parse_args(base).opening_plies is None
    assert play.parse_args(base + ["-r", "3"]).rounds == 3
    args = play.parse_args(base + ["-r", "4", "--opening-plies", "4"])
    assert (args.opening_plies, args.rounds) == (4, 4)
    assert play.parse_args(base + ["-r", "3", "--opening-plies", "0"]).opening_plies is None
    with pytest.raises(SystemExit):
        play.parse_args(base + ["-r", "3", "--opening-plies", "4"])
    assert "--rounds must be even" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        play.parse_args(base + ["-r", "4", "--opening-plies", "42"])
    assert "--opening-plies N must be" in capsys.readouterr().err

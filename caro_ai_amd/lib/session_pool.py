"""Many human-vs-bot games on ONE engine: what a chat front end keeps in place of its dictionary of `Session`s.

A `Session` (lib/play_session.py) owns a net, an `MCTS` and an engine with one game slot, and a bot move is one
search for one workgroup's worth of work.  Here a session is a SLOT of one lock-step `SelfPlayEngine`: the pool owns
one engine and one packed net, every slot is HELD (include/caro_hip.h, "session pool") except while its bot moves,
and `move_bots` searches every listed session in the same launches.

    pool = SessionPool(game, model_file, slots=256)
    sessions[user] = pool.open(player_moves_first)     # was: Session(game, model_file, player_moves_first)
    ...
    pool.move_bots([s for s in sessions.values() if s.bots_turn()])   # or s.move_bot() for one of them

Sessions need not play at one strength: `pool.open(..., level=Level(searches=10, tau=0.5, net=1))` gives a session its own
minibatch budget, move temperature and net (the pool takes up to two), and sessions of different levels are still
searched in the same launches (include/caro_hip.h, "session pool": LEVELS).

A `PooledSession` carries `Session`'s attributes and methods under the same names.  What differs from `Session`: the
Dirichlet rows of a search are the engine's generated ones, keyed (seed, uid, ply, simulation), so a session's moves are
a function of (seed, uid, the human's moves, its own levels) and of nothing else -- not of the other sessions or their
levels, not of the slot, not of numpy's global stream; `Session` keeps a seeded numpy stream in step with the reference instead."""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from caro_ai_amd import _lib
from caro_ai_amd import config as cfg
from caro_ai_amd.engine import SelfPlayEngine


LINE_ENDS = ("depth", "win", "draw", "leaf")  # caro_principal_lines' end codes 0..3 (include/caro_hip.h)


TAU_MIN, TAU_MAX = 0.05, 8.0  # a temperature is 0 or in this range (caro_engine_set_temperature's check)


class Level(NamedTuple):
    """How strongly the bot of one session plays.  `searches`: the minibatches of `pool.batch` simulations one bot move
    searches (None: the pool's own); `tau`: the temperature the move is sampled at from the root's visit counts (0: the
    most visited move); `net`: which of the pool's nets evaluates the session's leaves (0 or 1)."""
    searches: Optional[int] = None
    tau: float = 0.0
    net: int = 0

    def checked(self, n_nets=2) -> "Level":
        """the level with plain ints / a float, or ValueError"""
        searches, tau, net = self.searches, self.tau, self.net
        if searches is not None:
            if isinstance(searches, bool) or not isinstance(searches, (int, np.integer)):
                raise ValueError("Level: searches must be an integer or None, not %r" % (searches,))
            # (one minibatch on an unexpanded root backs nothing up: the root has no visits and the ply is refused)
            if int(searches) < 2:
                raise ValueError("Level: searches must be >= 2, not %r" % (searches,))
            searches = int(searches)
        try:
            tau = float(tau)
        except (TypeError, ValueError):
            raise ValueError("Level: tau must be a number, not %r" % (self.tau,))
        if not (tau == 0.0 or TAU_MIN <= tau <= TAU_MAX):  # (NaN fails both)
            raise ValueError("Level: tau must be 0 or in [%g, %g], not %r" % (TAU_MIN, TAU_MAX, self.tau))
        if isinstance(net, bool) or not isinstance(net, (int, np.integer)) or not 0 <= int(net) < n_nets:
            raise ValueError("Level: net must be an index in [0, %d), not %r" % (n_nets, net))
        return Level(searches, tau, int(net))


class Line(NamedTuple):
    """One variation of an `Analysis`: a root move and the most visited replies after it.  `values[d]` is the search's
    estimate of move d seen from the side that makes it (sides alternate from `Analysis.to_move`), formed as
    `PooledSession.value` is.  `end`: why the line stops -- "win" (the last move wins for its mover), "draw" (it fills
    the board), "depth" (the asked-for length), "leaf" (the search has not looked further)."""
    moves: Tuple[int, ...]
    visits: Tuple[int, ...]
    values: Tuple[float, ...]
    priors: Tuple[float, ...]
    end: str


class Analysis(NamedTuple):
    """What the session's kept tree says about its current position: the side to move, the visits below the root (None:
    the position has not been searched at all, `lines` is then empty) and the variations, most visited root move first."""
    to_move: int
    root_visits: Optional[int]
    lines: Tuple[Line, ...]

    def text(self) -> str:
        if not self.lines:
            return "no analysis: the position has not been searched"
        return "\n".join("%d. %s  visits %d  value %+.2f%s" % (
            i + 1, " ".join(str(m) for m in ln.moves), ln.visits[0], float(ln.values[0]),
            "" if ln.end in ("depth", "leaf") else "  (%s)" % ln.end) for i, ln in enumerate(self.lines))


class PooledSession:
    def __init__(self, pool, slot, uid, player_moves_first):
        game = pool.game
        self.pool, self.slot, self.uid = pool, slot, uid
        self.game = game
        self.BOT_PLAYER, self.USER_PLAYER = game.player_black, game.player_white
        self.model_file = pool.model_file
        self.player_moves_first = player_moves_first
        self.device = pool.device
        self.state = game.initial_state
        self.moves = []     # every move of the game, both sides, in order
        self.value = None   # the bot's own estimate of its last move
        self.finished = False
        self.closed = False
        self.to_move = self.USER_PLAYER if player_moves_first else self.BOT_PLAYER
        self._level = None  # None: the pool's own searches, the most visited move, the first net

    # what Session keeps per game lives in the pool: one net, one engine
    model = property(lambda self: self.pool.model)
    mcts_store = property(lambda self: self.pool.engine)

    level = property(lambda self: self._level)

    def set_level(self, level):
        """the session's `Level` from its next bot move on (None: back to the pool's own); between moves, at any time"""
        if self.closed:
            raise ValueError("set_level on a closed session")
        self.pool._set_level(self, level)

    def bots_turn(self) -> bool:
        return not self.closed and not self.finished and self.to_move == self.BOT_PLAYER

    def _play(self, move, who) -> bool:
        """put `who`'s token, remember the move; True when it wins the game"""
        self.moves.append(move)
        self.state, won = self.game.move(self.state, move, who)
        self.to_move = self.BOT_PLAYER if who == self.USER_PLAYER else self.USER_PLAYER
        self.finished = bool(won) or self.is_draw()
        return won

    def move_player(self, move: int) -> bool:
        if self.closed or self.finished:
            raise ValueError("move_player on a %s session" % ("closed" if self.closed else "finished"))
        if self.to_move != self.USER_PLAYER:
            raise ValueError("move_player out of turn: the bot is to move")
        if not self.is_valid_move(move):
            raise ValueError("illegal move %r" % (move,))
        won = self._play(int(move), self.USER_PLAYER)
        if not self.finished:  # the new root of the slot's search; its tree is kept
            self.pool.engine.pool_set([self.slot], [self.state], [self.BOT_PLAYER], [len(self.moves)])
        return won

    def move_bot(self) -> bool:
        return self.pool.move_bots([self])[0][2]

    def hint(self, searches=0, top=3, depth=8) -> "Analysis":
        """`SessionPool.analyse` of this session alone: the moves the bot considers here and the lines it expects"""
        return self.pool.analyse([self], searches=searches, top=top, depth=depth)[0]

    def is_valid_move(self, move: int) -> bool:
        return move in self.game.possible_moves(self.state)

    def is_draw(self) -> bool:
        return not self.game.possible_moves(self.state)

    def render(self) -> str:
        head = "" if self.value is None else "Position evaluation: %.2f\n" % float(self.value)
        return "%s<pre>%s</pre>" % (head, self.game.render(self.state))


class SessionPool:
    def __init__(self, game, model_file, slots=64, device="cuda:0", searches=cfg.BOT_MCTS_SEARCHES,
                 batch=cfg.BOT_MCTS_BATCH_SIZE, seed=0, evaluator=None, evict=None, node_cap=None, engine=None):
        """`model_file`: a checkpoint, or a sequence of two for sessions to choose from (`Level.net`); `models` /
        `model_files` hold all of them, `model` / `model_file` the first.
        `evaluator`: a ready device-side evaluator (net_hip.HashNet in the tests), or two, in place of the checkpoints.
        `evict`: None = on for the boards where lib.utils.play_games switches it on (searches x batch x cells above a
        default tree).  `engine`: a ready engine in place of the pool's own (the bookkeeping tests hand in a stub)."""
        self.game = game
        # one net, or two for sessions to choose from (Level.net): `model_file` / `evaluator` may be a sequence of two
        files = list(model_file) if isinstance(model_file, (list, tuple)) else [model_file]
        evaluators = (list(evaluator) if isinstance(evaluator, (list, tuple)) else [evaluator]) if evaluator is not None else None
        if not 1 <= len(files) <= 2 or (evaluators is not None and not 1 <= len(evaluators) <= 2):
            raise ValueError("SessionPool takes one net or two")
        self.model_files = files
        self.model_file = files[0]
        self.device = device
        self.searches, self.batch = int(searches), int(batch)
        self.n_slots = int(slots)
        self.models = []
        if engine is None:
            if evaluators is None:
                from caro_ai_amd.lib import model
                from caro_ai_amd.net_hip import HipNet
                for f in files:
                    weights = torch.load(f, map_location=lambda storage, loc: storage)
                    self.models.append(model.Net.from_state_dict(weights, input_shape=game.obs_shape,
                                                                 actions_n=game.action_space).eval())
                evaluators = [HipNet(m, str(device)) for m in self.models]
            cells = game.obs_shape[1] * game.obs_shape[2]
            if evict is None:
                evict = self.searches * self.batch * cells + 64 > SelfPlayEngine.DEFAULT_CAP_LIMIT
            engine = SelfPlayEngine(game, self.n_slots, evaluators=evaluators, n_stores=1, max_batch=self.batch,
                                    node_cap=node_cap, steps_before_tau_0=0, first_player_mode=0, c_puct=cfg.C_PUCT,
                                    alpha=cfg.ALPHA, explore=cfg.EXPLORE, seed=seed, device=device,
                                    searches_hint=self.searches, evict=bool(evict))
            if len(evaluators) == 2:
                # (two nets in one engine: the pool calls need session levels on -- a slot's net is then its own, net 0
                # until a Level says otherwise)
                engine.pool_level([], [], [])
            engine.pool_hold()  # a fresh engine's slots are live: nothing searches before a session is opened
        self.model = self.models[0] if self.models else None
        self.engine = engine
        self.evaluators = evaluators
        self.evaluator = evaluators[0] if evaluators else None
        self.n_nets = max(len(files), len(evaluators or ()))
        self._levels = len(evaluators or ()) == 2  # has pool_level ever gone out: move_bots then states budgets
        self._free = list(range(self.n_slots))  # lowest free slot first
        self._next_uid = 0
        self._overflows = 0

    def close_pool(self):
        self.engine.close()

    # ------------------------------------------------------------ sessions
    def open(self, player_moves_first, uid=None, level=None) -> PooledSession:
        if level is not None:
            level = Level(*level).checked(self.n_nets)
        if not self._free:
            raise RuntimeError("pool is full")
        if uid is None:
            uid = self._next_uid
        self._next_uid = max(self._next_uid, int(uid) + 1)
        slot = self._free.pop(0)
        s = PooledSession(self, slot, int(uid), player_moves_first)
        # empty trees, the initial position (the bot, if it moves first, is the player to move there), held
        self.engine.pool_open([slot], [s.uid], [s.to_move])
        if level is not None:
            self._set_level(s, level)
        return s

    def _set_level(self, session, level):
        if level is not None:
            level = Level(*level).checked(self.n_nets)
        if level is None and not self._levels:
            return  # nobody ever had a level: the engine is never told of them
        # (the engine keeps net and tau per slot; the budget goes out with every selection, see move_bots)
        self.engine.pool_level([session.slot], [level.net if level else 0], [level.tau if level else 0.0])
        self._levels = True
        session._level = level

    def _budget(self, session):
        level = session._level
        return self.searches if level is None or level.searches is None else level.searches

    def close(self, session):
        """frees the session's slot; the next open() that takes it clears it"""
        if session.closed or session.pool is not self:
            raise ValueError("close of a session that is not open in this pool")
        session.closed = True
        self._free.append(session.slot)
        self._free.sort()

    # ------------------------------------------------------------ the bot's moves
    def move_bots(self, sessions):
        """One bot move in every listed session: `searches` x `batch` simulations on each session's own kept tree and
        the ply, for exactly those slots, in one chain of launches.  Returns [(move, value, won)] in the order given and
        updates the sessions (state, moves, value).  In a pool with levels each session searches its own level's
        minibatches (the launches run to the largest of them), with its own net, and samples its move at its own tau."""
        sessions = list(sessions)
        seen = set()
        for s in sessions:
            if not isinstance(s, PooledSession) or s.pool is not self or s.closed:
                raise ValueError("move_bots: a listed session is closed or not of this pool")
            if s.finished:
                raise ValueError("move_bots: a listed session's game is over")
            if s.to_move != s.BOT_PLAYER:
                raise ValueError("move_bots: a listed session is not on the bot's turn")
            if s.slot in seen:
                raise ValueError("move_bots: a session is listed twice")
            seen.add(s.slot)
        if not sessions:
            return []
        eng = self.engine
        slots = [s.slot for s in sessions]
        if self._levels:
            budgets = [self._budget(s) for s in sessions]
            eng.pool_select_budget(slots, budgets)
            eng.search(max(budgets), self.batch)
        else:
            eng.pool_select(slots)
            eng.search(self.searches, self.batch)
        rows = eng.lookup_dev(slots, [0] * len(slots), [s.state for s in sessions])  # the searched roots, before the ply moves on
        actions, done, _ = eng.step()
        eng.pool_hold()
        overflows = eng.counters()["overflows"]  # the host waits here, once, for everything above
        if overflows > self._overflows:
            self._overflows = overflows
            raise _lib.CaroError("SessionPool: the node pool of a session overflowed or a ply was refused "
                                 "(node_cap=%d): the move is not the search's" % eng.cfg.node_cap)
        idx = torch.as_tensor(slots, dtype=torch.int64).to(actions.device)
        act = actions[idx].cpu().numpy()
        over = done[idx].cpu().numpy()
        rows = {k: v.cpu().numpy() for k, v in rows.items()}
        out = []
        for i, s in enumerate(sessions):
            move = int(act[i])
            if move < 0 or not rows["found"][i]:
                raise _lib.CaroError("SessionPool: slot %d made no ply" % s.slot)
            n = int(rows["N"][i][move])
            # Q[move] as MCTS.get_policy_value reports it: the float32 Q word once a net value has been backed up
            # through the edge, the exact W / N before that
            value = (np.float32(rows["Q"][i][move]) if rows["strong"][i][move]
                     else (float(rows["W"][i][move]) / n if n else 0.0))
            s.value = value
            won = s._play(move, s.BOT_PLAYER)
            if bool(over[i]) != s.finished:
                raise _lib.CaroError("SessionPool: slot %d and the host disagree about the end of the game" % s.slot)
            out.append((move, value, won))
        return out

    # ------------------------------------------------------------ what the bot thinks
    def analyse(self, sessions, searches=0, top=3, depth=8):
        """The `top` most visited moves of every listed session's current position and the line the search expects
        after each, at most `depth` moves, read out of the session's kept tree on the device in one launch
        (caro_principal_lines, include/caro_hip.h).  Either side may be to move: on the human's turn it is a hint.
        Returns one `Analysis` per session, in the order given.

        searches = 0 reads only: nothing about a session changes and the bot's later moves are what they would have
        been.  searches > 0 PONDERS first -- `searches` x `batch` simulations from the current position with the usual
        noise key (seed, uid, ply = moves so far, sim); the visits stay in the session's kept tree, so its later bot moves
        are a function of (seed, uid, the human's moves, the analyse calls with searches > 0).  On the bot's turn, in a
        session not analysed before, the first move of the first line and its value are what `move_bots` with the same
        `searches` would play and report."""
        sessions = list(sessions)
        seen = set()
        for s in sessions:
            if not isinstance(s, PooledSession) or s.pool is not self or s.closed:
                raise ValueError("analyse: a listed session is closed or not of this pool")
            if s.finished:
                raise ValueError("analyse: a listed session's game is over")
            if s.slot in seen:
                raise ValueError("analyse: a session is listed twice")
            seen.add(s.slot)
        if int(searches) < 0:
            raise ValueError("analyse: searches must be >= 0")
        if not sessions:
            return []
        eng = self.engine
        slots = [s.slot for s in sessions]
        # the slot's root IS the session's position, with its side to move, at ply = len(moves): by pool_open before the
        # first move, by move_player's pool_set on the bot's turn, by the bot's own ply on the human's
        eng.pool_select(slots)
        if int(searches) > 0:
            eng.search(int(searches), self.batch)
        rows = eng.principal_lines(slots, int(top), int(depth))
        eng.pool_hold()
        overflows = eng.counters()["overflows"]  # the host waits here, once, for everything above
        if overflows > self._overflows:
            self._overflows = overflows
            raise _lib.CaroError("SessionPool: the node pool of a session overflowed "
                                 "(node_cap=%d): the analysis is not the search's" % eng.cfg.node_cap)
        rows = {k: v.cpu().numpy() for k, v in rows.items()}
        out = []
        for i, s in enumerate(sessions):
            visits = int(rows["root_visits"][i])
            lines = []
            for j in range(int(rows["n_lines"][i])):
                n = int(rows["len"][i][j])
                N, W, Q = rows["N"][i][j][:n], rows["W"][i][j][:n], rows["Q"][i][j][:n]
                strong = rows["strong"][i][j][:n]
                # as move_bots forms `value`: the float32 Q word once a net value went through the edge, else W / N
                values = tuple(np.float32(Q[d]) if strong[d] else float(W[d]) / int(N[d]) for d in range(n))
                lines.append(Line(moves=tuple(int(a) for a in rows["move"][i][j][:n]), visits=tuple(int(x) for x in N),
                                  values=values, priors=tuple(float(p) for p in rows["P"][i][j][:n]),
                                  end=LINE_ENDS[int(rows["end"][i][j])]))
            out.append(Analysis(to_move=s.to_move, root_visits=None if visits < 0 else visits, lines=tuple(lines)))
        return out

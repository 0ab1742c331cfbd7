"""The reference of caro_principal_lines (include/caro_hip.h, "position analysis") in pure Python, over ANY tree that can
answer `get_node(state) -> {"N", "W", "Q", "P", "W_is_f32"} | None` (the oracle's get_node, or a dict of hand-written
rows).  It imports nothing of the code under test: the rules come in as `game` (`move`, `possible_moves`)."""

DEPTH, WIN, DRAW, LEAF = 0, 1, 2, 3
END_NAMES = ("depth", "win", "draw", "leaf")


def _first_max(N):
    """the edge with the largest N, ties to the lowest action (np.argmax's rule); None if no edge has a visit"""
    best = None
    for a in range(len(N)):
        if int(N[a]) > 0 and (best is None or int(N[a]) > int(N[best])):
            best = a
    return best


def _step(node, a):
    return {"move": a, "N": int(node["N"][a]), "W": float(node["W"][a]), "Q": float(node["Q"][a]),
            "P": float(node["P"][a]), "strong": int(bool(node["W_is_f32"][a]))}


def principal_lines(game, get_node, state, player, top, depth):
    """-> {"root_visits": int (-1: the root is no node), "lines": [{"steps": [step, ...], "end": code}]}; a step is
    {"move", "N", "W", "Q", "P", "strong"} with W, Q, P as Python floats of the stored words"""
    assert 1 <= top <= 16 and 1 <= depth <= 64
    root = get_node(state)
    if root is None:
        return {"root_visits": -1, "lines": []}
    A = len(root["N"])
    visited = [a for a in range(A) if int(root["N"][a]) > 0]
    ranked = sorted(visited, key=lambda a: (-int(root["N"][a]), a))
    lines = []
    for head in ranked[:top]:
        steps, node, a, pos, who = [], root, head, state, player
        while True:
            steps.append(_step(node, a))
            pos, won = game.move(pos, a, who)
            if won:
                end = WIN
            elif not game.possible_moves(pos):
                end = DRAW
            elif len(steps) == depth:
                end = DEPTH
            else:
                node = get_node(pos)
                a = _first_max(node["N"]) if node is not None else None
                end = LEAF if a is None else None
            if end is not None:
                break
            who = 1 - who
        lines.append({"steps": steps, "end": end})
    return {"root_visits": sum(int(n) for n in root["N"]), "lines": lines}

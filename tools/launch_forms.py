#!/usr/bin/env python3
"""Two moves in every launch form of the engine's search, under three option states: the workload whose kernel-name ->
launch-count table says WHICH instantiation of each tree kernel the host side launches.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/launch_forms.py
    python tools/prof_summary.py ...   (or read DIR/*_kernel_stats.csv: Name, Calls)

Forms: Connect4 at batch 8 (one wavefront per game: k_tree), Connect4 at batch 4 (step-wise: k_select, k_encode,
k_expand_backup), 3 x 3 m,n,k at batch 8 (several wavefronts per game: k_tree_mw), and the two fused ones staggered
(k_tree_stag, k_tree_stag_mw).  Option states: nothing set (the lean form where it exists), first-play urgency (full),
virtual loss 2 (TreeVl in the launches that select).  Each engine searches and moves twice (`caro_search_move`, or two
staggered passes) with the table net and drains after each move.  A host-side refactor must leave the table unchanged.
Prints one line per (form, options) with the engine's counters, so that two runs can also be compared by result."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

G, SEARCHES, MOVES = 4, 3, 2


def main():
    import torch
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.game.tictactoe import TicTacToe
    from caro_ai_amd.net_hip import HashNet
    assert torch.cuda.is_available(), "needs a GPU"
    forms = (("c4 batch 8", ConnectFour, 8, False), ("c4 batch 4 step-wise", ConnectFour, 4, False),
             ("mnk 3x3 batch 8", TicTacToe, 8, False), ("c4 batch 8 staggered", ConnectFour, 8, True),
             ("mnk 3x3 batch 8 staggered", TicTacToe, 8, True))
    options = (("none", lambda e: None), ("fpu", lambda e: e.set_fpu(0.5, 0.25)), ("vl 2", lambda e: e.set_virtual_loss(2)))
    for name, make_game, batch, stagger in forms:
        for opt, apply in options:
            game = make_game()
            net = HashNet(game, device="cuda:0")
            eng = SelfPlayEngine(game, G, evaluators=[net], max_batch=batch, seed=3, device="cuda:0",
                                 searches_hint=SEARCHES, stagger=stagger)
            apply(eng)
            for _ in range(MOVES):
                if stagger:
                    eng.search(SEARCHES, batch)
                else:
                    eng.search_step(SEARCHES, batch)
                eng.drain()
            torch.cuda.synchronize()
            c = eng.counters()
            print("%-28s %-5s kernel_form %d  sims %d  levels %d" % (name, opt, eng.kernel_form(), c["sims"], c["levels"]))
            eng.close()
            net.close()


if __name__ == "__main__":
    main()

"""CPU model of the payload barrier `pf_sum_barrier` (csrc/pf_grid.h) that the multi-workgroup EMD kernels meet at: each of G
workgroups adds (value << 32 | 1) to a 64-bit word in one atomic, then polls the word until it holds every arrival of the
barrier and takes the value sum from the same read.  Arrive and poll are atomic steps; every interleaving of G = 2 and 3
workgroups over 3 barriers is enumerated.  With two words alternating by barrier parity every workgroup reads the same
per-barrier total.  With one word (the running sum emd_repl_kernel used before) a workgroup that has passed barrier k adds its
next value before a slower one has read barrier k's total - the model must find that interleaving, or it could not see the race."""
import pytest

NBAR = 3


def _value(w, k):
    return (k + 1) * (w + 1)                              # non-zero and different per workgroup and barrier


def _finals(G, parity):
    """-> {per-workgroup tuples of the totals each barrier returned: one entry per reachable end state}."""
    start = ((0,) * G, (0, 0), ((0, 0),) * G, ((),) * G)  # program counters, words, each workgroup's last sums, results
    stack, visited, finals = [start], set(), set()
    while stack:
        st = stack.pop()
        if st in visited:
            continue
        visited.add(st)
        pcs, words, seen, res = st
        if all(pc == 2 * NBAR for pc in pcs):
            finals.add(res)
            continue
        for w in range(G):
            pc = pcs[w]
            if pc == 2 * NBAR:
                continue
            nb = pc // 2 + 1                              # barrier number 1, 2, ...
            i = nb & 1 if parity else 0
            npcs = pcs[:w] + (pc + 1,) + pcs[w + 1:]
            if pc % 2 == 0:                               # arrive: one 64-bit atomic add
                nwords = list(words)
                nwords[i] += (_value(w, nb) << 32) | 1
                stack.append((npcs, tuple(nwords), seen, res))
            else:                                         # poll: one atomic load; a read that is still short changes nothing
                target = ((nb + 1) >> 1) * G if parity else nb * G
                v = words[i]
                if (v & 0xffffffff) < target:
                    continue
                s = v >> 32
                total = s - seen[w][i]
                nseen = list(seen[w])
                nseen[i] = s
                stack.append((npcs, words, seen[:w] + (tuple(nseen),) + seen[w + 1:], res[:w] + (res[w] + (total,),) + res[w + 1:]))
    return finals


@pytest.mark.parametrize("G", [2, 3])
def test_parity_words_give_every_workgroup_the_same_total(G):
    finals = _finals(G, parity=True)
    want = tuple(sum(_value(w, k) for w in range(G)) for k in range(1, NBAR + 1))
    assert finals == {(want,) * G}


@pytest.mark.parametrize("G", [2, 3])
def test_one_word_lets_a_run_ahead_arrival_into_a_slower_read(G):
    finals = _finals(G, parity=False)
    assert any(len(set(res)) > 1 for res in finals)      # two workgroups of one launch saw different totals

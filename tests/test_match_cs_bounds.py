"""The matches tests/test_gpu_match_cs.py runs at the layout's upper bound, 64 players, and the property that makes them worth running.

At 64 players the walk of the step kernel has 63 steps; step i exchanges positions i and rem_i = stream output (i - 1) mod (i + 1).
Which of a step's three cases a match takes -- the self-exchange rem_i == i, the exchange with position 0, rem_i == 0, or an exchange
with a position strictly between -- is decided by the stream cipher, so at a late step the two rare cases (one in i + 1 each) do not
turn up in a handful of random matches.  directed_matches() searches (seed, random) pairs through the restatement's stream cipher, in a
fixed order and under a cap, and keeps a pair whenever it takes a case of a watched step that no pair kept so far takes.  That the kept
matches cover every case of every watched step is a property of the inputs alone: it is asserted here, without a device, and the GPU
test runs the very same matches."""
import anemoi_ref as an
import match_cs_ref as mr
from test_match_cs_ref_host import match

PLAYERS = mr.MAX_PLAYERS
STEPS = [1, 31, 32, 62, 63]          # the first step; both sides of the half wave; the last two, which read lanes 62 and 63
CASES = ["self", "zero", "between"]
SEARCH_CAP = 256                     # pairs tried at the most (75 ms each); the search below ends after 51
_FOUND = []


def remainders(seed, random_number, players=PLAYERS):
    """[players]: rem_i of step i (entry 0 is no step)"""
    stream = an.eval_stream_cipher([seed, random_number], players - 1)
    return [0] + [stream[i - 1] % (i + 1) for i in range(1, players)]


def case_of(step, rem):
    assert 0 <= rem <= step
    return "self" if rem == step else "zero" if rem == 0 else "between"


def wanted():
    """every (step, case) that exists: at step 1 the remainder is 0 or 1, nothing lies between"""
    return {(i, c) for i in STEPS for c in CASES if not (c == "between" and i < 2)}


def directed_matches():
    """(matches, the (step, case) pairs they take, how many pairs the search tried): found once, shared by both test modules"""
    if not _FOUND:
        missing, kept, tried = wanted(), [], 0
        while missing and tried < SEARCH_CAP:
            seed, rnd = 1 + tried, 2 * tried + 1             # small and distinct: the cipher does the mixing
            rem = remainders(seed, rnd)
            new = {(i, case_of(i, rem[i])) for i in STEPS} & missing
            if new:
                missing -= new
                kept.append((match(PLAYERS, "directed-%d" % tried)[0], seed, rnd))
            tried += 1
        _FOUND.append((kept, wanted() - missing, tried))
    return _FOUND[0]


def test_the_directed_matches_take_every_case_of_every_watched_step():
    ms, _, tried = directed_matches()
    assert tried == 51 <= SEARCH_CAP and len(ms) == 9
    seen = set()
    for inputs, seed, rnd in ms:
        assert len(inputs) == PLAYERS == 64 and len(set(inputs)) == PLAYERS    # distinct inputs: a wrong index is a wrong value
        rem = remainders(seed, rnd)
        # the remainders are the restated circuit's own, not only this file's reading of the cipher
        cs = mr.build_cs(inputs, seed, rnd)
        assert [cs.witness[v] for v, d in enumerate(cs.defs) if d[0] == mr.REM] == rem[1:]
        seen |= {(i, case_of(i, rem[i])) for i in STEPS}
    assert seen == wanted() and len(wanted()) == 3 * len(STEPS) - 1

"""The exchange of the persistent trend kernel's partial sums (option "trend_exchange", chicdiff_amd/csrc/trend_kernels.hip): every
double leaves its workgroup as two 64-bit words, (tag << 32) | low half and (tag << 32) | high half, tag = pass + 1, and a reader
takes a word only when it carries the tag of the pass it is summing — no fence, no counter.  The packing and the accept rule are
plain functions of fit_state.h (xchg_pack, xchg_unpack, xchg_accept), compiled for the host as well
(chicdiff_hip_selftest_trend_exchange).  Checked here, without a GPU: the round trip of every kind of double, the accept rule, and
a model of the protocol — a few workgroups, single-word stores and loads in every order the protocol permits — in which every
reader must end up with exactly the writers' values of its pass; with one buffer instead of two the model must find a reader that
can never finish."""
import ctypes as C
import struct

import numpy as np
import pytest

TAGS = [1, 2, 2 ** 10, 2 ** 32 - 1]
PACK, UNPACK, ACCEPT = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip.load_library()


def call(L, op, tag, n, x=None, words=None, accept=None):
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    rc = L.chicdiff_hip_selftest_trend_exchange(op, tag, n, ptr(x, C.c_double), ptr(words, C.c_uint64), ptr(accept, C.c_int32))
    assert rc == 0, rc


def pack(L, x, tag):
    x = np.ascontiguousarray(x, np.float64)
    words = np.zeros(2 * len(x), np.uint64)
    call(L, PACK, tag, len(x), x=x, words=words)
    return words


def unpack(L, words, tag):
    words = np.ascontiguousarray(words, np.uint64)
    x = np.zeros(len(words) // 2, np.float64)
    ok = np.zeros(len(words) // 2, np.int32)
    call(L, UNPACK, tag, len(x), x=x, words=words, accept=ok)
    return x, ok


def accepts(L, words, tag):
    words = np.ascontiguousarray(words, np.uint64)
    ok = np.zeros(len(words), np.int32)
    call(L, ACCEPT, tag, len(words), words=words, accept=ok)
    return ok


def special_bits():
    bits = [0x0000000000000000, 0x8000000000000000,                      # +-0
            0x7ff0000000000000, 0xfff0000000000000,                      # +-inf
            0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000001,  # quiet / signalling NaNs with payloads
            0x7ff7ffffffffffff, 0xffffffffffffffff, 0x7ff80000deadbeef,
            0x0000000000000001, 0x800fffffffffffff, 0x0000000100000000,  # denormals
            0x7fefffffffffffff, 0xffefffffffffffff,                      # the largest finite double
            0x0010000000000000, 0x3ff0000000000000, 0x00000000ffffffff, 0xffffffff00000000]
    rng = np.random.default_rng(20261020)
    rnd = rng.integers(0, 2 ** 64, size=100_000, dtype=np.uint64)
    return np.concatenate([np.array(bits, np.uint64), rnd])


@pytest.mark.parametrize("tag", TAGS)
def test_round_trip_keeps_every_bit(lib, tag):
    bits = special_bits()
    x = bits.view(np.float64)
    words = pack(lib, x, tag)
    # the layout the kernel's readers rely on: tag in the upper half of both words, the double's halves in the lower halves
    assert np.array_equal(words >> np.uint64(32), np.full(len(words), tag, np.uint64))
    assert np.array_equal(words[0::2] & np.uint64(0xffffffff), bits & np.uint64(0xffffffff))
    assert np.array_equal(words[1::2] & np.uint64(0xffffffff), bits >> np.uint64(32))
    back, ok = unpack(lib, words, tag)
    assert back.view(np.uint64).tobytes() == bits.tobytes()
    assert ok.all()


def test_accept_rule_wants_the_very_tag_in_both_words(lib):
    x = np.array([0.0, -0.0, 1.5, np.inf, np.nan, 5e-324, 1.7976931348623157e308])
    every = TAGS + [0, 3, 2 ** 10 - 1, 2 ** 10 + 1, 2 ** 31, 2 ** 32 - 2]
    for want in every:
        for have in every:
            if have == 0:
                words = np.repeat(x.view(np.uint64) & np.uint64(0xffffffff), 2)  # never written: tag 0 whatever the payload
            else:
                words = pack(lib, x, have)
            ok = accepts(lib, words, want)
            assert ok.all() if (have == want and want != 0) else not ok.any(), (want, have)
            if have != 0 and want != 0 and have != want:  # one word of the pair right, the other one stale: the pair is refused
                good = pack(lib, x, want)
                for mixed in (np.where(np.arange(len(words)) % 2 == 0, good, words), np.where(np.arange(len(words)) % 2 == 1, good, words)):
                    _, pair_ok = unpack(lib, mixed, want)
                    assert not pair_ok.any(), (want, have)
    # a double that another kernel left behind can never pass for a word of tag 0, and the zero fill is refused for every tag
    assert not accepts(lib, special_bits()[:1000], 0).any()
    for tag in TAGS:
        assert not accepts(lib, np.zeros(4, np.uint64), tag).any()


# ---- the protocol, as a model ------------------------------------------------------------------------------------------------------------
# W workgroups run PASSES passes.  In pass p a workgroup stores the two words of its value into its slot of buffer p & 1 (one buffer
# when the parity rule is off) and loads both words of every workgroup's slot, its own included; a load that the accept rule refuses
# changes nothing and is simply made again.  The stores of pass p + 1 depend on every value of pass p (the state step), so they
# follow the last accepted load of pass p; nothing else is ordered: a workgroup's two stores may land in either order, its loads may
# be accepted in ANY order (every lane of the kernel polls on its own), and they run beside its stores.  Events are single words.
# Every reachable state is visited, at W = 2 and at W = 3 (2 765 337 states with two buffers), by two walkers:
#   Model   one state at a time, the memory words kept in the state as they are stored — the plain statement, used at W = 2;
#   Walker  all states of one depth at a time, as numpy arrays — the same events; what a slot holds is read off its owner's progress
#           (only the owner stores there, its two words each once per pass).  test_the_two_walkers_agree holds it against Model.
# Every event moves exactly one workgroup one step forward, so the states are layered by the number of events so far, nothing is
# ever revisited from a later layer, and every run in which whoever can move eventually does ends in a state without moves: the
# property "nobody waits forever" is that the only such state is the one where all have finished.

PASSES = 4


def value(b, p):
    """what workgroup b publishes in pass p: distinct in both halves from every other (b, p)"""
    return struct.unpack("<d", struct.pack("<II", 0x1000 + 16 * p + b, 0x40000000 + 256 * p + b))[0]


class Model:
    def __init__(self, L, W, parity):
        self.L, self.W, self.parity = L, W, parity
        self.words = {(b, p): tuple(int(w) for w in pack(L, [value(b, p)], p + 1)) for b in range(W) for p in range(PASSES)}
        self.cache = {}

    def accept(self, word, tag):
        key = (word, tag)
        if key not in self.cache:
            self.cache[key] = bool(accepts(self.L, np.array([word], np.uint64), tag)[0])
        return self.cache[key]

    def buf(self, p):
        return p & 1 if self.parity else 0

    def start(self):
        wg = tuple((0, 0, 0) for _ in range(self.W))          # per workgroup: pass, stores landed (2 bits), loads accepted (2 W bits)
        mem = tuple(0 for _ in range(2 * self.W * 2))          # [buffer][workgroup][word], zero-filled
        return wg, mem

    def moves(self, state):
        """every event that changes the state: (next state, wrong) — wrong: an accepted word that is not the writer's word of that pass"""
        wg, mem = state
        W = self.W
        full = (1 << (2 * W)) - 1
        for me, (p, smask, lmask) in enumerate(wg):
            if p == PASSES:
                continue

            def advanced(smask2, lmask2):
                nxt = (p + 1, 0, 0) if smask2 == 3 and lmask2 == full else (p, smask2, lmask2)
                return wg[:me] + (nxt,) + wg[me + 1:]

            for i in range(2):
                if not smask >> i & 1:
                    at = (self.buf(p) * W + me) * 2 + i
                    yield (advanced(smask | 1 << i, lmask), mem[:at] + (self.words[(me, p)][i],) + mem[at + 1:]), False
            for j in range(2 * W):  # any pending load, in any order
                if lmask >> j & 1:
                    continue
                b, i = divmod(j, 2)
                word = mem[(self.buf(p) * W + b) * 2 + i]
                if self.accept(word, p + 1):
                    yield (advanced(smask, lmask | 1 << j), mem), word != self.words[(b, p)][i]

    def explore(self):
        """(states, wrong acceptances, states with nothing left to happen in which somebody has not finished — as workgroup tuples)"""
        first = self.start()
        seen, todo, wrong, stuck = {first}, [first], 0, []
        while todo:
            s = todo.pop()
            nxt = list(self.moves(s))
            if not nxt and any(p != PASSES for p, _, _ in s[0]):
                stuck.append(s[0])
            for t, bad in nxt:
                wrong += bad
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return len(seen), wrong, stuck


class Walker:
    """The same model, a whole layer of states per step.  A state is one integer: per workgroup a field of loads accepted (2 W bits),
    stores landed (2 bits) and pass (3 bits)."""

    def __init__(self, L, W, parity):
        self.W, self.parity = W, parity
        self.nl = 2 * W
        self.fw = self.nl + 5
        # word[b][i][t]: what word i of workgroup b's slot holds when its last store there carried tag t (0: the zero fill)
        self.word = np.zeros((W, 2, PASSES + 1), np.uint64)
        for b in range(W):
            for p in range(PASSES):
                self.word[b, :, p + 1] = pack(L, [value(b, p)], p + 1)
        # the library's accept rule for every such word and every tag a reader can ask for
        self.acc = np.zeros((W, 2, PASSES + 1, PASSES + 1), bool)
        for want in range(1, PASSES + 1):
            self.acc[..., want] = accepts(L, self.word.reshape(-1), want).reshape(W, 2, PASSES + 1) != 0

    def fields(self, S, k):
        f = (S >> (k * self.fw)) & ((1 << self.fw) - 1)
        return f >> (self.nl + 2), (f >> self.nl) & 3, f & ((1 << self.nl) - 1)  # pass, stores landed, loads accepted

    def decode(self, s):
        return tuple(tuple(int(x[0]) for x in self.fields(np.array([s], np.int64), k)) for k in range(self.W))

    def holds(self, S, b, i, p_reader):
        """the tag in word i of workgroup b's slot in the buffer a reader in pass p_reader looks at.  Only b stores there: in its
        pass pb, word i once.  Two buffers: the buffer of pb holds tag pb + 1 once that store has landed and before it what pass
        pb - 2 left (tag pb - 1, or the zero fill), the other buffer what pass pb - 1 left (tag pb, or the zero fill)."""
        pb, smb, _ = self.fields(S, b)
        landed = ((smb >> i) & 1) == 1
        if not self.parity:
            return np.where(landed, pb + 1, pb)
        same = ((pb ^ p_reader) & 1) == 0
        return np.where(same, np.where(landed, pb + 1, np.where(pb >= 2, pb - 1, 0)), pb)

    def explore(self):
        W, nl, fw = self.W, self.nl, self.fw
        full = (1 << nl) - 1
        S = np.zeros(1, np.int64)
        states, wrong, stuck = 0, 0, []
        while len(S):
            states += len(S)
            moved = np.zeros(len(S), bool)
            done = np.ones(len(S), bool)
            nxt = []
            for me in range(W):
                p, sm, lm = self.fields(S, me)
                live = p < PASSES
                done &= ~live
                rest = S & ~np.int64(((1 << fw) - 1) << (me * fw))

                def emit(can, sm2, lm2):
                    f = np.where((sm2 == 3) & (lm2 == full), (p + 1) << (nl + 2), (p << (nl + 2)) | (sm2 << nl) | lm2)
                    nxt.append((rest | (f << (me * fw)))[can])
                    moved[can] = True

                for i in range(2):
                    emit(live & (((sm >> i) & 1) == 0), sm | (1 << i), lm)
                want = np.minimum(p + 1, PASSES)
                for j in range(nl):
                    b, i = divmod(j, 2)
                    t = self.holds(S, b, i, p)
                    can = live & (((lm >> j) & 1) == 0) & self.acc[b, i, t, want]
                    wrong += int(np.sum(can & (self.word[b, i, t] != self.word[b, i, want])))
                    emit(can, sm, lm | (1 << j))
            stuck.extend(self.decode(s) for s in S[~moved & ~done][:4])
            S = np.unique(np.concatenate(nxt)) if nxt else S[:0]
        return states, wrong, stuck


def stranded(wg, W):
    """in a state without moves: a reader that waits for tag p + 1 in a slot (the one buffer) whose owner has already stored a later
    pass's word there — it can never complete"""
    for p, _, lmask in wg:
        for j in range(2 * W):
            pb, smb, _ = wg[j // 2]
            holds = pb + 1 if smb >> (j % 2) & 1 else pb
            if p < PASSES and not lmask >> j & 1 and holds > p + 1:
                return True
    return False


@pytest.mark.parametrize("parity", [True, False])
def test_the_two_walkers_agree(lib, parity):
    """Walker reads a slot's content off its owner's progress instead of keeping the memory: at W = 2 it must visit as many states
    as Model, which keeps it, and reach the same verdicts"""
    a_states, a_wrong, a_stuck = Model(lib, 2, parity).explore()
    b_states, b_wrong, b_stuck = Walker(lib, 2, parity).explore()
    assert a_states == b_states and a_wrong == b_wrong == 0 and bool(a_stuck) == bool(b_stuck) == (not parity)
    if not parity:
        assert set(b_stuck) <= set(a_stuck)


@pytest.mark.parametrize("W", [2, 3])
def test_every_interleaving_delivers_the_pass_values(lib, W):
    """two buffers by pass parity: in every reachable state somebody can still move until all have finished (every event moves the
    state forward, so every fair run ends), and no reader ever accepts anything but the writer's word of its pass"""
    states, wrong, stuck = (Model if W == 2 else Walker)(lib, W, True).explore()
    print(W, "workgroups:", states, "states")
    assert states > 1000 and wrong == 0 and not stuck
    if W == 3:
        assert states == 2765337  # every order of the loads: 9 865 if a workgroup's loads were taken in slot order only


@pytest.mark.parametrize("W", [2, 3])
def test_one_buffer_strands_a_reader(lib, W):
    """the parity rule carries weight: with one buffer a workgroup that runs ahead overwrites a word a slower one still waits for,
    and that reader can never complete (what it does accept is still never wrong: the tags see to that)"""
    states, wrong, stuck = (Model if W == 2 else Walker)(lib, W, False).explore()
    print(W, "workgroups, one buffer:", states, "states,", len(stuck), "stuck states kept")
    assert wrong == 0 and stuck
    assert all(stranded(wg, W) for wg in stuck)

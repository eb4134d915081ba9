"""TEST INFRASTRUCTURE for the live-transcript entry points (include/binius_amd_host.h, "Against a live transcript"): a Python
challenger whose every sample depends on everything observed so far, and the bookkeeping of a schedule -- the alternation of writes
and draws a phase makes, which the tests compute from the shapes alone.

The challenger is NOT the reference's HasherChallenger<Groestl256> and does not need to be: it only has to make every sample a function
of every earlier message byte.  Its state is SHA-256 over an 8-byte draw counter followed by all MESSAGE bytes so far, expanded to
16 bytes per scalar (or masked to `bits` for sample_bits).  DECOMMITMENT bytes are recorded and not absorbed.

A schedule is a list of events
    ("w", channel, n_bytes)      a write segment
    ("s", role, n)               n samples of B128; role names the array of the array form they belong to
    ("b", n)                     n x sample_bits
Neighbouring events of one kind merge when a log is compared: only the concatenation between two draws is specified."""
import hashlib

MESSAGE, DECOMMITMENT = 0, 1


class Hasher:
    """the challenger alone: observe(bytes), sample() -> int below 2^128, sample_bits(bits)"""

    def __init__(self):
        self.observed, self.draws = bytearray(), 0

    def observe(self, data):
        self.observed += data

    def _block(self):
        h = hashlib.sha256(self.draws.to_bytes(8, "little") + bytes(self.observed)).digest()
        self.draws += 1
        return h

    def sample(self):
        return int.from_bytes(self._block()[:16], "little")

    def sample_bits(self, bits):
        return int.from_bytes(self._block()[:8], "little") & ((1 << bits) - 1)


def make_challenger(base):
    """The challenger as a subclass of binius_amd._host.Transcript (imported by the caller: CPU-only tests may not have the library)."""

    class Challenger(base):
        def __init__(self, slow_at=None, fail_at=None, fail_with=None):
            base.__init__(self)
            self.h = Hasher()
            self.written = {MESSAGE: bytearray(), DECOMMITMENT: bytearray()}
            self.log = []        # ("w", channel, n_bytes) | ("s", n) | ("b", n), as called
            self.drawn, self.drawn_bits = [], []
            self.segments = []   # the MESSAGE bytes between two draws, one entry per write call
            self.slow_at, self.fail_at, self.fail_with = slow_at, fail_at, fail_with
            self.sample_calls = 0

        def write(self, channel, data):
            self.written[channel] += data
            self.log.append(("w", channel, len(data)))
            if channel == MESSAGE:
                self.h.observe(data)

        def sample(self, n):
            call = self.sample_calls
            self.sample_calls += 1
            if call == self.fail_at:
                raise self.fail_with
            if call == self.slow_at:
                import time

                time.sleep(0.02)
            out = [self.h.sample() for _ in range(n)]
            self.drawn += out
            self.log.append(("s", n))
            return out

        def sample_bits(self, bits, n):
            out = [self.h.sample_bits(bits) for _ in range(n)]
            self.drawn_bits += out
            self.log.append(("b", n))
            return out

    return Challenger


def merged(events):
    """events with neighbours of one kind (and channel) summed; roles dropped: [("w", channel, bytes) | ("s", n) | ("b", n)]"""
    out = []
    for e in events:
        if e[0] == "w":
            key, count = ("w", e[1]), e[2]
        elif e[0] == "s":
            key, count = ("s",), e[-1]
        else:
            key, count = ("b",), e[-1]
        if count == 0:
            continue
        if out and out[-1][0] == key:
            out[-1][1] += count
        else:
            out.append([key, count])
    return [k + (c,) for k, c in out]


def roles_of(schedule, drawn):
    """the drawn samples dealt to the roles of the schedule, in drawing order: {role: [ints]}"""
    roles, at = {}, 0
    for e in schedule:
        if e[0] == "s":
            roles.setdefault(e[1], [])
            roles[e[1]] += drawn[at : at + e[2]]
            at += e[2]
    assert at == len(drawn), "the schedule draws %d samples, the transcript served %d" % (at, len(drawn))
    return roles


def zero_roles(schedule):
    return roles_of(schedule, [0] * sum(e[2] for e in schedule if e[0] == "s"))


def scalars(values):
    """write_scalar_slice: 16 little-endian bytes per element"""
    return b"".join(int(v).to_bytes(16, "little") for v in values)


def replay(schedule, message, bits=0):
    """The verifier's side of Fiat-Shamir: a fresh challenger reads the recorded MESSAGE bytes segment by segment and draws at the
    schedule's points.  Returns ({role: samples}, [sample_bits values])."""
    h, at, roles, idx = Hasher(), 0, {}, []
    for e in schedule:
        if e[0] == "w":
            if e[1] == MESSAGE:
                h.observe(message[at : at + e[2]])
                at += e[2]
        elif e[0] == "s":
            roles.setdefault(e[1], [])
            roles[e[1]] += [h.sample() for _ in range(e[2])]
        else:
            idx += [h.sample_bits(bits) for _ in range(e[1])]
    assert at == len(message)
    return roles, idx

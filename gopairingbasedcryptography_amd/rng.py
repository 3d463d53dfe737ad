"""The randomness of the batched Encrypt / KeyGenerate planners, drawn where the batch lives: engine.fr_random over one 32-byte seed
(include/gpbc_bn254_random.h: a ChaCha20 block per scalar, reduced modulo r on the device).  Replaces the caller-side
fr.Element.SetRandom() per scalar of the reference (cpabe/bsw07/bsw07_cpabe.go, utils/generate_random_polynomial.go,
fibe/sw05_fibe_common.go:205-210) and the half gigabyte of host-made scalars a 2^16 x 256 BSW07 Encrypt would otherwise upload.

Every draw of one Randomness takes the NEXT stream id, starting at 0, and reads that stream from index 0 in row-major order, so two
draws never share a block and a scalar's value depends on (seed, draw number, position) alone: the *_seeded planners document the order
of their draws, which makes a ciphertext reproducible from a seed.  The seed is KEY MATERIAL — whoever holds it can recompute every
scalar drawn, the s of every ciphertext among them — so it is never shown by repr() and never put into an error message.
Engine-agnostic like the planners: the engine is an argument."""
import secrets

import numpy as np

from . import _buffers as bufs

SEED_BYTES = 32


class Randomness:
    """Randomness(engine, seed=None): seed is 32 bytes; None draws them from secrets.token_bytes.

        rng = Randomness(engine, seed)
        s = rng.scalars(messages, n)             # [n, 32], stream 0, indices 0 .. n - 1, of the kind of `messages`
        c = rng.scalars(messages, n, C)          # [n, C, 32], stream 1, index i C + j for entry (i, j)
        rng.next_stream                          # 2: the stream id the next draw takes
    """

    def __init__(self, engine, seed=None):
        if seed is None:
            seed = secrets.token_bytes(SEED_BYTES)
        if not isinstance(seed, (bytes, bytearray)) or len(seed) != SEED_BYTES:
            raise ValueError("seed must be %d bytes" % SEED_BYTES)
        self._engine, self._seed, self._next = engine, bytes(seed), 0

    @property
    def next_stream(self):
        return self._next

    def scalars(self, like, *shape):
        """[*shape, 32] scalars in [0, r) of the kind of `like` (a numpy array, or a CUDA tensor: a tensor on its device, enqueued on
        the current stream).  Takes the next stream id and reads it from index 0 in row-major order; a draw of no scalars (an extent
        of 0) takes no stream id."""
        if not shape or any(not isinstance(e, (int, np.integer)) or isinstance(e, bool) or e < 0 for e in shape):
            raise ValueError("shape must be one or more non-negative integers")
        shape = tuple(int(e) for e in shape)
        n = 1
        for e in shape:
            n *= e
        if not n:
            return bufs.empty(tuple(shape) + (32,), like)
        if self._next >> 64:
            raise ValueError("this Randomness has used all 2^64 streams")
        out = self._engine.fr_random(self._seed, n, stream=self._next, first=0, like=like)
        self._next += 1
        return bufs.view(out, *shape, 32)

    def __repr__(self):
        return "Randomness(next_stream=%d)" % self._next

"""The synthetic cases the chord grammar's GPU kernel tests run (tests/test_gpu_chord_grammar_kernels.py), kept apart from them so that the
CPU suite can judge the same cases with the restatement alone (tests/test_chord_grammar_ref_host.py: the skippable share, obeys)."""
import functools

import numpy as np

import chord_grammar_ref as CG
import chord_sample_ref as CS

SEED, DRAW = 11, 4                                           # those of tests/test_gpu_chord_decode_kernels.py
TEMPERATURES = ((1.0, 0.7), (1.0, 0.0), (0.0, 0.5))
TRIADS = [0x091, 0x089, 0x049, 0x111]
SEVENTHS = TRIADS + [0x891, 0x491, 0x489, 0x449, 0x249, 0x889]
MAJOR = 0xab5


def vocabulary(V):
    """V distinct templates that hold interval 0: the sevenths first, then the odd 12-bit numbers in ascending order"""
    out = list(SEVENTHS)
    x = 1
    while len(out) < 64:
        if x not in out:
            out.append(x)
        x += 2
    return out[:V]


def logits(B, seed, scale=2.0):
    """N(0, scale) logits as the plain chord kernel tests draw them"""
    rng = np.random.RandomState(seed)
    return (rng.normal(0, scale, (B, 12)).astype(np.float32), rng.normal(0, scale, (B, 12, 2)).astype(np.float32),
            rng.normal(0, scale, (B, 12)).astype(np.float32))


def rule_table(B, t=0):
    """int32 [B]: the words of B rows at one step -- a key per row (b % 12, major), and by b % 6: vocabulary with both flags | the key's
    masks alone | both flags without a vocabulary | a vocabulary without a mask | the identity | roots I, IV, V of the key with vocabulary
    and chord-tone bass"""
    b = np.arange(B)
    key = (b + t) % 12
    scale = CG.rot12(MAJOR, key)
    prim = CG.rot12(0x0a1, key)
    kind = b % 6
    w = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                  [scale | scale << 12 | CG.VOCAB | CG.ROOT_IN_CHORD | CG.BASS_IN_CHORD, scale | scale << 12,
                   scale | scale << 12 | CG.ROOT_IN_CHORD | CG.BASS_IN_CHORD, CG.IDENTITY | CG.VOCAB | CG.ROOT_IN_CHORD, CG.IDENTITY],
                  prim | scale << 12 | CG.VOCAB | CG.BASS_IN_CHORD)
    return w.astype(np.int32)


@functools.lru_cache(maxsize=None)
def sampled_case(Tc, Th, B=512, t=5, offset=1000, V=17):
    """one sampled case: logits, the restated noise of the samples offset .. offset + B - 1, the per-row rule table, V templates"""
    lg = logits(B, 2)
    g = offset + np.arange(B)
    case = dict(B=B, t=t, offset=offset, logits=lg, nz=CS.noise(SEED, DRAW, g, t), vz=CG.vocab_noise(SEED, DRAW, g, t, V), rule=rule_table(B, t),
                vocab=np.array(vocabulary(V), np.int32))
    for v in case.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return case

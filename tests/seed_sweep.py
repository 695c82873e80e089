"""Generator seeds across the whole 64-bit range, in every kernel that seeds a generator.

include/ptrace.h takes four ``uint64_t`` seeds; PT_PCG_PIXEL gives pixel ``i = row * W + col`` the generator
``PCG(S0, Q0 + i)``, PT_PCG_SAMPLE gives sample ``k`` of it ``PCG(S0, Q0 + i * nsamp + k)``, PT_PCG_SEQ enters the one stream
``PCG(jitter_state, jitter_seq)`` at draw ``2 * nsamp * i``.  The sum is written out at each seeding site on its own, so a
32-bit temporary at one of them renders a plausible, wrong frame that no small seed shows.  Here catalogue cases
(tests/variant_catalog.py: worlds, sizes, cameras, tunings and planned kernels unchanged) are rendered under seed pairs
whose sum crosses 2^32, 2^63 (where ``(seq << 1) | 1`` drops the top bit) and 2^64 (where it wraps) INSIDE the frame:

    name       state                  seq, PIXEL / SAMPLE      seq, SEQ
    hi-state   2^32 + 45              54                       54
    x32        2^64 - 1               2^32 - c                 2^32 + 54
    x63        2^63 + 12345           2^63 - c                 2^63 - 1
    x64        0x9E3779B97F4A7C15     2^64 - c                 2^64 - 1

``c`` is the generator index of the crossing pixel, a pixel in the middle of the rows the case renders (of the rank's rows
for a share): ``gpix`` under PIXEL, ``gpix * nsamp`` under SAMPLE, ``gpix`` the GLOBAL pixel index.  Every pixel before it in
row-major order has a sequence number below the boundary, the crossing pixel and every later one a number at or beyond it.
Under SEQ the pair goes into ``jitter_state`` / ``jitter_seq`` and the path seeds hold values that must play no part; in
the other modes it is the reverse.

Seeding sites and the cases that reach them (P: PIXEL, S: SAMPLE, Q: SEQ):

    pt_simple.h:98   pcg_seed_pixel   P simple-pointlight-hoist, simple-flat-ortho-jitter
                                      Q simple-flat-hoist-jitter, simple-pointlight-hoist, simple-flat-ortho-jitter (SEQ)
    pt_simple.h:105  per sample       S simple-flat-hoist-jitter (nsamp 4)
    pt_tile.h:830    pcg_seed_pixel   P tile-onoff-jitter, tile-flat-hier-jitter-share (a rank's rows), tile-flat-ortho-jitter
                                      Q tile-onoff-jitter, tile-pointlight, tile-flat-ortho-jitter, tile-pointlight-ortho (SEQ)
    pt_tile.h:840    per sample       S tile-pointlight (nsamp 1), tile-pointlight-ortho (nsamp 4)
    pt_hits.h:107    pcg_seed_pixel   P, Q tests/test_gpu_seeds.py: the hit frames
    pt_hits.h:113    per sample       S the hit frames
    pt_path.h:393    one lane         P sw-cull-0-path
    pt_path.h:396    one lane         S path-one-lane (nsamp 1)
    pt_path.h:413    regions / queue  S regions-lds-scene-lean-centre-sample (S = 0, nsamp 1), flagged-lean-lds-handover (nsamp 4)
    pt_path.h:819    regions / queue  P regions-lds-scene-lean, regions-hbm-deep, flagged-lean-lds-queue, flagged-split-handover
    pt_tree.h:272    tree             P tree-lean-scene, tree-lean-scene-share-rb5 (a rank's rows); behind a hand-over:
                                        flagged-split-handover
    pt_tree.h:303    tree, per sample S tree-balls (nsamp 1); behind a hand-over: flagged-lean-lds-handover (nsamp 4)
    pt_math.h        pcg_seed_pixel   every P and Q row above that names it

The state travels on through the regions kernel's shuffles and speculation (the regions cases), the hand-over record (the
two hand-over cases) and ``pcg_advance`` (the SEQ cases: ``pcg_advance64``; the tree cases).

tile-pointlight-ortho is added to the issue's list: tile-pointlight has one sample per pixel, so the factor ``nsamp`` of
pt_tile.h:840 would otherwise be 1 wherever the tile kernel seeds per sample.  tile-flat-hier-jitter-share has no SEQ
variant: the oracle's serial loop walks a rank's rows only, so it is no judge of a share of a SEQ frame.

A plain helper module: no fixtures, no hooks.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from pytracer_amd import abi
from tests import variant_catalog as vc

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1

SIMPLE = ["simple-flat-hoist-jitter", "simple-pointlight-hoist", "simple-flat-ortho-jitter"]
TILE = ["tile-onoff-jitter", "tile-pointlight", "tile-flat-hier-jitter-share", "tile-flat-ortho-jitter", "tile-pointlight-ortho"]
PATH = ["path-one-lane", "sw-cull-0-path",
        "regions-lds-scene-lean", "regions-lds-scene-lean-centre-sample", "regions-hbm-deep",
        "tree-lean-scene", "tree-lean-scene-share-rb5", "tree-balls",
        "flagged-lean-lds-queue", "flagged-lean-lds-handover", "flagged-split-handover"]
CASE_IDS = SIMPLE + TILE + PATH
# the jittered non-path cases that also run under the SEQ alignment (whole frames only, see above)
SEQ_CASE_IDS = [cid for cid in SIMPLE + TILE if vc.params(vc.BY_ID[cid]).n_ranks == 1]

# name -> (state, the boundary the sum crosses under PIXEL / SAMPLE or None, seq under SEQ)
PAIRS = {
    "hi-state": (2**32 + 45, None, 54),
    "x32": (2**64 - 1, 2**32, 2**32 + 54),
    "x63": (2**63 + 12345, 2**63, 2**63 - 1),
    "x64": (0x9E3779B97F4A7C15, 2**64, 2**64 - 1),
}
SEED_NAMES = list(PAIRS)
CROSSING_NAMES = ["x32", "x63", "x64"]
# what the seeds that play no part are set to (the jitter seeds under PIXEL / SAMPLE, the path seeds under SEQ)
UNUSED = (0x0123456789ABCDEF, 2**40 + 3)

# every (case id, seed name, mode or None) the sweep renders; mode None: the case's own PIXEL / SAMPLE
SWEEP = [(cid, name, None) for cid in CASE_IDS for name in SEED_NAMES] + \
        [(cid, name, abi.PCG_SEQ) for cid in SEQ_CASE_IDS for name in SEED_NAMES]


def sweep_id(cid: str, name: str, mode: Optional[int]) -> str:
    return f"{cid}-{name}" + ("-seq" if mode == abi.PCG_SEQ else "")


def nsamp(p: abi.Params) -> int:
    return max(int(p.samples_per_side), 1) ** 2


def crossing_pixel(case: vc.Case) -> Tuple[int, int]:
    """(row, col) of the crossing pixel: the middle column of the middle one of the rows the case renders (global row)."""
    rows = vc.rows(case)
    return rows[len(rows) // 2], case.size[0] // 2


def crossing_index(p: abi.Params, row: int, col: int) -> int:
    """The generator index ``c`` of pixel (row, col): what the device adds to ``path_seq`` for its first generator."""
    gpix = row * int(p.width) + col
    return gpix * nsamp(p) if p.pcg_mode == abi.PCG_SAMPLE else gpix


def seeds(case: vc.Case, name: str, mode: Optional[int] = None) -> Tuple[int, int]:
    """(state, seq) of pair ``name`` for ``case``: both in [0, 2^64)."""
    state, boundary, seq_seq = PAIRS[name]
    base = vc.params(case)
    if mode == abi.PCG_SEQ:
        return state, seq_seq
    assert mode is None or mode == base.pcg_mode
    if boundary is None:
        return state, 54
    c = crossing_index(base, *crossing_pixel(case))
    assert 0 < c < 2**32
    return state, (boundary - c) & M64


def with_seeds(base: abi.Params, state: int, seq: int) -> abi.Params:
    """``base`` with (state, seq) as the seeds its ``pcg_mode`` reads and ``UNUSED`` as the others."""
    if base.pcg_mode == abi.PCG_SEQ:
        return abi.copy_params(base, jitter_state=state, jitter_seq=seq, path_state=UNUSED[0], path_seq=UNUSED[1])
    return abi.copy_params(base, path_state=state, path_seq=seq, jitter_state=UNUSED[0], jitter_seq=UNUSED[1])


def params(case: vc.Case, name: str, mode: Optional[int] = None) -> abi.Params:
    """The catalogue's params of ``case`` with only the seeds (and, for a SEQ variant, ``pcg_mode``) replaced."""
    base = vc.params(case)
    if mode == abi.PCG_SEQ:
        base = abi.copy_params(base, pcg_mode=abi.PCG_SEQ)
    return with_seeds(base, *seeds(case, name, mode))


def contrast_seeds(case: vc.Case, name: str, mode: Optional[int] = None) -> List[Tuple[str, Tuple[int, int]]]:
    """The seeds a frame under pair ``name`` must differ from: (a) the catalogue's (45, 54), (b) the pair reduced mod 2^32
    -- for x63 the pair with ``seq + 1`` instead -- and (c) the pair with ``seq + 2^32``."""
    state, seq = seeds(case, name, mode)
    b = ("seq+1", (state, (seq + 1) & M64)) if name == "x63" else ("mod 2^32", (state & M32, seq & M32))
    return [("(45, 54)", (45, 54)), b, ("seq+2^32", (state, (seq + 2**32) & M64))]

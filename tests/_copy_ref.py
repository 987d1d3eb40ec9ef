"""Inputs and expected outputs of the copy-collective tests (tests/test_copy_cpu.py, tests/test_copy_gpu.py).

Plain CPU torch: no torch.distributed, no project code. Payloads are bytes (tensors of other dtypes are views
of them). `inputs` gives every rank's input chunks from seeds, so any rank regenerates everyone's; `expected`
is one routing rule per collective, written as index arithmetic -- it knows nothing of tiles, owners, staging
or any other part of a protocol. `explain` turns a mismatch into one line that names the tile, the vector and
the place in the inputs where the wrong bytes came from.
"""
import torch

from tests import _exact as E

T = 4096  # the tile every engine moves (kern::kTileBytes); used only to describe and to mutate, never to route
COLLS = ("broadcast", "all_gather", "gather", "scatter", "all_to_all", "all_to_all_uneven")


def chunks_of(coll, world):
    """Input chunks per rank."""
    return 1 if coll in ("broadcast", "all_gather", "gather") else world


def chunk_bytes(coll, nbytes, q):
    """Bytes of input chunk q: `nbytes`, except in the uneven all-to-all, where every rank sends q + 1 rows
    of `nbytes` bytes to rank q."""
    return (q + 1) * nbytes if coll == "all_to_all_uneven" else nbytes


def inputs(coll, nbytes, world, seed):
    """[rank][chunk] -> uint8 tensor, full-range random bits, a distinct seed per (rank, chunk).
    broadcast: one chunk per rank (the root's is the payload, the others' are what their tensors hold before
    the call); all_gather / gather: one chunk per rank; scatter / all_to_all: `world` chunks per rank."""
    assert coll in COLLS, coll
    return [[E.random_bits(chunk_bytes(coll, nbytes, q), torch.uint8, (seed * 64 + r) * 64 + q)
             for q in range(chunks_of(coll, world))] for r in range(world)]


def constant_inputs(coll, nbytes, world):
    """The payload the older tests use: one constant per (rank, chunk), as torch.full gives."""
    nc = chunks_of(coll, world)
    return [[torch.full((chunk_bytes(coll, nbytes, q),), 1 + r * nc + q, dtype=torch.uint8) for q in range(nc)]
            for r in range(world)]


def expected(coll, inputs, rank, root):
    """The bytes every output tensor of `rank` holds after the call, in output order ([] for a rank that
    receives nothing)."""
    world = len(inputs)
    if coll == "broadcast":      # out = the root's tensor, on every rank (the root included: it is unchanged)
        return [inputs[root][0]]
    if coll == "all_gather":     # out[q] = rank q's input
        return [inputs[q][0] for q in range(world)]
    if coll == "gather":         # the same on the root, nothing elsewhere
        return [inputs[q][0] for q in range(world)] if rank == root else []
    if coll == "scatter":        # out = chunk `rank` of the root's list
        return [inputs[root][rank]]
    if coll in ("all_to_all", "all_to_all_uneven"):  # out[q] = chunk `rank` of rank q's list
        return [inputs[q][rank] for q in range(world)]
    raise ValueError(coll)


def flat(chunks):
    return torch.cat([c.reshape(-1) for c in chunks]) if chunks else torch.empty(0, dtype=torch.uint8)


def identical(got, want):
    """The comparison of every test: byte for byte, no tolerance."""
    return bool(got.dtype == want.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want))


def distinct_vectors(inputs):
    """(rows, distinct rows) of all ranks' input chunks cut into 16-byte vectors; where a chunk ends past its
    last whole vector its last 16 bytes are one more row, and a chunk below 16 bytes is one row as a whole."""
    rows, seen = 0, set()
    whole = []
    for per_rank in inputs:
        for c in per_rank:
            n = c.numel() // 16 * 16
            if n:
                whole.append(c[:n].view(-1, 16))
                if c.numel() - n:
                    whole.append(c[-16:].view(1, 16))
            elif c.numel():
                rows += 1
                seen.add(bytes(c.tolist()))
    tails = len(seen)
    vec = 0
    if whole:
        allv = torch.cat(whole)
        rows += allv.shape[0]
        # rows whose first 8 bytes are all distinct are distinct (one sort of int64); otherwise compare whole rows
        vec = torch.unique(allv.view(torch.int64)[:, 0]).numel()
        if vec != allv.shape[0]:
            vec = torch.unique(allv, dim=0).shape[0]
    return rows, vec + tails


def _find(inputs, needle):
    for r, per_rank in enumerate(inputs):
        for q, c in enumerate(per_rank):
            at = c.numpy().tobytes().find(needle)
            if at >= 0:
                return r, q, at
    return None


def explain(got, want, inputs, sources):
    """One line about the first differing byte of the outputs `got` (lists of uint8 tensors, as `expected`
    returns them). `sources[k]` = (rank, chunk) that output k is routed from."""
    for k, (g, w) in enumerate(zip(got, want)):
        if g.numel() != w.numel():
            return f"output {k}: {g.numel()} bytes, want {w.numel()}"
        bad = (g != w).nonzero().flatten()
        if bad.numel() == 0:
            continue
        off = int(bad[0])
        line = (f"{bad.numel()} of {w.numel()} bytes of output {k} differ, first at +{off} (tile {off // T}, "
                f"vector {off % T // 16}, byte {off % 16}; source rank {sources[k][0]} chunk {sources[k][1]}); "
                f"got {g[off:off + 4].tolist()} want {w[off:off + 4].tolist()}")
        v0 = off // 16 * 16
        needle = bytes(g[v0:v0 + 16].tolist())
        if len(needle) == 16:
            hit = _find(inputs, needle)
            if hit:
                line += (f"; the got-bytes at +{v0} are rank {hit[0]} chunk {hit[1]} offset {hit[2]} of the inputs "
                         f"(tile {hit[2] // T}, vector {hit[2] % T // 16})")
            elif not bool(g[v0:v0 + 16].any()):
                line += "; the got-bytes are zero"
            else:
                line += "; the got-bytes are nowhere in the inputs"
        return line
    if len(got) != len(want):
        return f"{len(got)} outputs, want {len(want)}"
    return ""


# ------------------------------------------------------------------------------------------ mutations
# What a subtly wrong engine would deliver, applied to the expected outputs of one rank. Each returns a new list
# of output chunks, or None where the collective has nothing to mutate that way. tests/test_copy_cpu.py asserts
# that `identical` rejects every one of them on `inputs`, and that it does not on `constant_inputs`.
def _mut_swap_tiles(coll, ins, rank, root, world):
    out = [c.clone() for c in expected(coll, ins, rank, root)]
    c = out[-1]
    if c.numel() < 2 * T:
        return None
    c[:T], c[T:2 * T] = c[T:2 * T].clone(), c[:T].clone()
    return out


def _mut_swap_ranks(coll, ins, rank, root, world):
    if coll == "broadcast":  # another rank's tensor arrives
        return expected(coll, ins, rank, (root + 1) % world)
    if coll == "scatter":    # another rank's chunk arrives
        return expected(coll, ins, (rank + 1) % world, root)
    out = list(expected(coll, ins, rank, root))
    if coll == "all_to_all_uneven":  # (every output of a rank has the same length there)
        assert out[0].numel() == out[1].numel()
    out[0], out[1] = out[1], out[0]
    return out


def _mut_rotate_owner(coll, ins, rank, root, world):
    # inside every chunk, each whole row of `world` tiles rotated by one tile (tile t is owned by rank t % W in
    # the 2-shot broadcast, and the pulls of the other collectives rotate over the peers from tile to tile)
    out = [c.clone() for c in expected(coll, ins, rank, root)]
    hit = False
    for c in out:
        rows = c.numel() // (world * T)
        if rows:
            v = c[:rows * world * T].view(rows, world, T)
            v.copy_(torch.roll(v, 1, dims=1).clone())
            hit = True
    return out if hit else None


def _mut_shift16(coll, ins, rank, root, world):
    out = [torch.roll(c, 16) for c in expected(coll, ins, rank, root)]
    return out if any(c.numel() > 16 for c in out) else None


def _mut_zero_ragged(coll, ins, rank, root, world):
    out = [c.clone() for c in expected(coll, ins, rank, root)]
    hit = False
    for c in out:
        if c.numel() % T and c.numel() > T:
            c[c.numel() // T * T:] = 0
            hit = True
    return out if hit else None


def _mut_seam(coll, ins, rank, root, world):
    # the zero-copy body taken as whole rows of W tiles where the rest starts after whole tiles: the tiles
    # between the two seams are delivered from one seam too early
    out = [c.clone() for c in expected(coll, ins, rank, root)]
    hit = False
    for c in out:
        n = c.numel()
        by_tile, by_row = n // T * T, n // (world * T) * (world * T)
        if by_row and by_tile > by_row:
            c[by_row:n] = torch.cat([c[by_tile:n], c[by_row:by_tile]])
            hit = True
    return out if hit else None


MUTATIONS = {"swap_tiles": _mut_swap_tiles, "swap_ranks": _mut_swap_ranks, "rotate_owner": _mut_rotate_owner,
             "shift16": _mut_shift16, "zero_ragged": _mut_zero_ragged, "seam": _mut_seam}

"""numpy restatement of the GPU builder (real-time-gpu-ray-tracer_amd/csrc/lbvh.hip, lbvh_*.hpp) — TEST
INFRASTRUCTURE ONLY, the checker of RT_BUILD_LBVH trees.

The builder is this repository's own (the reference builds on the host only, src/AS/BLAS.cu:4-117),
so there is no reference output to pin it to; what is pinned is that every GPU-built tree equals the
tree this module derives from the same items, bit for bit:

  * item boxes are the reference's primitive boxes (oracle_prim_bounds, BoundingBox.cuh:24-55) and
    item centroids the reference's centroids (Triangle.cuh:53-61, Parallelogram.cuh:45-47);
  * 30-bit Morton codes of the centroids quantised to 1024 cells per axis of the tree's centroid
    bounds, float32 arithmetic in the kernel's order ((c - lo) / ext * 1024);
  * a stable sort by code; the binary radix tree over the sorted codes (Karras 2012), equal codes
    split by position; a subtree of <= cap items is one leaf;
  * output in the reference's node form: node 0 = root, an interior node's children are adjacent
    (left, left + 1) and allocated when the node is expanded, left subtree first (DFS leaf order).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def _clz32(x: int) -> int:
    return 32 - int(x).bit_length()


def _expand10(v: np.ndarray) -> np.ndarray:
    v = v.astype(np.uint64)
    v = (v * 0x00010001) & 0xFF0000FF
    v = (v * 0x00000101) & 0x0F00F00F
    v = (v * 0x00000011) & 0xC30C30C3
    v = (v * 0x00000005) & 0x49249249
    return v.astype(np.uint32)


INACTIVE_CODE = 0xFFFFFFFF


def morton_codes(cents: np.ndarray, active=None) -> np.ndarray:
    """active (bool per item, None = all): an inactive item (a TLAS record kept out of the tree, morton_kernel's
    centroid w != 0) is left out of the centroid bounds and gets the code 0xFFFFFFFF, behind every 30-bit code."""
    c = np.asarray(cents, F32)
    live = np.ones(c.shape[0], bool) if active is None else np.asarray(active, bool)
    codes = np.full(c.shape[0], INACTIVE_CODE, np.uint32)
    if not live.any():
        return codes
    c = c[live]
    lo, hi = c.min(axis=0), c.max(axis=0)
    q = np.zeros(c.shape, np.uint32)
    for a in range(3):
        ext = F32(hi[a] - lo[a])
        if not ext > 0:
            continue
        x = ((c[:, a] - lo[a]) / ext * F32(1024.0)).astype(F32)
        qa = np.where(x > 0, np.minimum(np.floor(x), 1023), 0)
        q[:, a] = np.where(x >= 1023, 1023, qa).astype(np.uint32)
    codes[live] = (_expand10(q[:, 0]) << 2) | (_expand10(q[:, 1]) << 1) | _expand10(q[:, 2])
    return codes


def lbvh_tree(boxes: np.ndarray, cents: np.ndarray, cap: int, active=None):
    """-> (node_boxes[n,6] f32, node_count_index[n,2] u32, refs[items] u32) in reference form;
    refs are item indices (0-based positions in `boxes`).  active: see morton_codes; an inactive item's box is
    taken as given (the builder's callers make it all +inf, launch_instance_update's inf_inactive)."""
    boxes = np.asarray(boxes, F32).reshape(-1, 6)
    n = boxes.shape[0]
    codes = morton_codes(cents, active)
    order = np.argsort(codes, kind="stable")
    keys = [int(k) for k in codes[order]]

    def delta(a, b):
        if keys[a] != keys[b]:
            return _clz32(keys[a] ^ keys[b])
        return 32 + _clz32(a ^ b)

    def split(first, last):            # Karras 2012 findSplit: last index sharing > common prefix
        common = delta(first, last)
        s, step = first, last - first
        while True:
            step = (step + 1) >> 1
            ns = s + step
            if ns < last and delta(first, ns) > common:
                s = ns
            if step <= 1:
                break
        return s

    def union(first, last):
        b = boxes[order[first:last + 1]]
        out = np.empty(6, F32)
        out[0::2] = b[:, 0::2].min(axis=0)
        out[1::2] = b[:, 1::2].max(axis=0)
        return out

    nodes_box, nodes_ci, refs = [np.zeros(6, F32)], [[0, 0]], []
    todo = [(0, n - 1, 0)]
    while todo:
        first, last, node = todo.pop()
        nodes_box[node] = union(first, last)
        if last - first + 1 <= cap:
            nodes_ci[node] = [last - first + 1, len(refs)]
            refs.extend(int(i) for i in order[first:last + 1])
            continue
        g = split(first, last)
        left = len(nodes_box)
        nodes_box += [np.zeros(6, F32), np.zeros(6, F32)]
        nodes_ci += [[0, 0], [0, 0]]
        nodes_ci[node] = [0, left]
        todo.append((g + 1, last, left + 1))
        todo.append((first, g, left))
    return np.asarray(nodes_box, F32), np.asarray(nodes_ci, np.uint32), np.asarray(refs, np.uint32)


def check_tree(node_boxes, ci, refs, item_boxes, cap):
    """Structural invariants of a reference-form tree: children adjacent, leaves <= cap, every item
    in exactly one leaf, every box the exact union of what it bounds.  Returns the height."""
    item_boxes = np.asarray(item_boxes, F32).reshape(-1, 6)
    assert sorted(int(r) for r in refs) == list(range(item_boxes.shape[0]))

    def union(bs):
        out = np.empty(6, F32)
        out[0::2] = bs[:, 0::2].min(axis=0)
        out[1::2] = bs[:, 1::2].max(axis=0)
        return out

    height = 0
    todo = [(0, 0)]
    while todo:
        j, d = todo.pop()
        cnt, idx = int(ci[j, 0]), int(ci[j, 1])
        if cnt:
            assert cnt <= cap
            assert np.array_equal(node_boxes[j], union(item_boxes[refs[idx:idx + cnt]])), j
            height = max(height, d)
            continue
        assert np.array_equal(node_boxes[j], union(node_boxes[idx:idx + 2])), j
        todo += [(idx, d + 1), (idx + 1, d + 1)]
    return height


def assert_tree_equal(got, want, what=None):
    """Two trees in reference form are the same bytes: topology (count / index), leaf order, node boxes."""
    nb, ci, refs = got
    wb, wci, wrefs = want
    assert np.array_equal(ci, wci), what
    assert np.array_equal(refs, wrefs), what
    assert np.array_equal(nb, wb), what

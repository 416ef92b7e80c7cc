"""What lmpc_store_retain leaves behind, restated in plain Python (test infrastructure): the reference of csrc/lmpc_retain.h and of the stores after the gather
kernel of csrc/lmpc_retain.hip.h.

  check_keep     what a keep list must look like: strictly ascending indices in [0, stored)
  keep_map       map[old] = new index, -1 for a dropped lap
  remap          indices that name laps under the new numbering, negative sentinels passed through; a named lap that is dropped is an error
  capacity       the lap capacity after a retain: the smallest initial * 2^j that holds the kept laps
  retain         tests/store_ref.RefStores after a retain: the kept laps of each store, in their order
  lap_bytes      bytes one lap slot of both stores and the prefilter image costs
"""
import numpy as np

CHUNK = 1024          # K1_CHUNK: rows of one image chunk


def check_keep(keep, stored):
    """None for a good list, else the position of the first entry that breaks the rule."""
    for k, v in enumerate(keep):
        if v < 0 or v >= stored or (k > 0 and v <= keep[k - 1]):
            return k
    return None


def keep_map(keep, stored):
    m = np.full(stored, -1, np.int32)
    for k, v in enumerate(keep):
        m[v] = k
    return m


def remap(indices, m):
    out = []
    for i in np.asarray(indices).reshape(-1).tolist():
        if i >= 0 and (i >= len(m) or m[i] < 0):
            raise ValueError("lap %d is named and not kept" % i)
        out.append(int(m[i]) if i >= 0 else i)
    return np.array(out, np.int32).reshape(np.asarray(indices).shape)


def capacity(initial, need):
    cap = int(initial)
    while cap < need:
        cap *= 2
    return cap


def retain(ref, ss=None, model=None):
    """tests/store_ref.RefStores `ref` after store_retain(ss, model), in place; returns (map_ss, map_model), None for an untouched store."""
    ms = mm = None
    if ss is not None:
        assert check_keep(ss, len(ref.ss)) is None
        ms = keep_map(ss, len(ref.ss)); ref.ss = [ref.ss[k] for k in ss]
    if model is not None:
        assert check_keep(model, len(ref.model)) is None
        mm = keep_map(model, len(ref.model)); ref.model = [ref.model[k] for k in model]
    return ms, mm


def lap_bytes(max_lap_len):
    """One lap slot of both stores (9 columns of doubles each), the three image planes of words and six doubles per image chunk."""
    chunks = (max_lap_len + CHUNK - 1) // CHUNK
    return 2 * 9 * max_lap_len * 8 + 3 * max_lap_len * 4 + chunks * 48

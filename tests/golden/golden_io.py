"""Golden archives larger than a committed file may be (1 MiB) are stored in parts, split by key in the original key
order: NAME_part1.npz, NAME_part2.npz, ...  load(NAME) reads them back as one archive (`.files` and `[key]`, like the
object np.load returns for a single .npz); save(NAME, arrays) writes them (tests/golden/make_golden*.py)."""
import glob
import io
import os
import re
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PART_LIMIT = 1000 * 1024        # bytes of compressed arrays per part, below the 1 MiB limit with room for the zip directory


def _parts(name):
    found = glob.glob(os.path.join(HERE, name + "_part*.npz"))
    num = {p: re.search(r"_part(\d+)\.npz$", p) for p in found}
    return sorted((p for p in found if num[p]), key=lambda p: int(num[p].group(1)))


class Golden:
    def __init__(self, paths):
        self._parts = [np.load(p) for p in paths]
        self.files = [k for z in self._parts for k in z.files]
        self._where = {k: z for z in self._parts for k in z.files}
        assert len(self._where) == len(self.files), "a key is stored in more than one part"

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where

    def keys(self):
        return list(self.files)


def load(name):
    paths = _parts(name)
    if not paths:
        raise FileNotFoundError(os.path.join(HERE, name + "_part1.npz"))
    return Golden(paths)


def save(name, arrays):
    """Write `arrays` (an ordered mapping) as NAME_part1.npz, ... each within PART_LIMIT; returns the paths."""
    groups, cur, size = [], {}, 0
    for k, v in arrays.items():
        buf = io.BytesIO()
        np.save(buf, np.asarray(v), allow_pickle=False)
        n = len(zlib.compress(buf.getvalue())) + 2 * len(k) + 200
        assert n <= PART_LIMIT, "%s alone is larger than a part may be" % k
        if cur and size + n > PART_LIMIT:
            groups.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    groups.append(cur)
    for p in _parts(name):
        os.remove(p)
    paths = []
    for i, g in enumerate(groups, 1):
        paths.append(os.path.join(HERE, "%s_part%d.npz" % (name, i)))
        np.savez_compressed(paths[-1], **g)
    return paths

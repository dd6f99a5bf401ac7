"""Cases shared by test_xbd_trainset_cpu.py and test_xbd_trainset_gpu.py: the class table of the resident labels
(dh_xbd_class_table_u8), the scripts' split and their oversampled index lists (datasets/xbd_pipeline).

    script_unet_train_indices   xBD_code/train_unettransformer.py:513-520, the loop as the script has it
    script_train_indices        xBD_code/train.py:397-425, the loop as the script has it, the doubled 'AOI' rows included
    class_rows                  random file_classes rows with a row of every kind forced in
    table_np                    the class table in numpy: np.bincount per file
    label_cases                 the byte patterns the kernel is tested with, for one shape
    known_sources               12 small sources whose labels hold known classes
"""
import functools

import numpy as np

CHUNK = 65536                   # dh_xbd_class_table_chunk(): the bytes of one file that one workgroup counts
# (n, hw): one byte; the three sizes around one 16-byte piece; files whose starts are not 16-aligned (17, 4099 are odd); the three
# sizes around one chunk; two chunks and a ragged third; a megabyte, where a counter packed into a byte or 16 bits would wrap
SHAPES = ((1, 1), (1, 15), (1, 16), (1, 17), (3, 17), (2, 4099), (3, CHUNK - 1), (2, CHUNK), (2, CHUNK + 1), (2, 2 * CHUNK + 33),
          (2, 1024 * 1024))
END_CLASSES = (1, 2, 3, 4, 200)


def script_unet_train_indices(file_classes, train_idxs0):
    """the script's loop, step by step: one list, appended to in the order of train_idxs0"""
    picked = []
    for i in train_idxs0:                                                       # 514
        picked.append(i)                                                        # 515: always
        if file_classes[i, 1:].max():                                           # 516: any of classes 2 .. 4
            picked.append(i)
        if file_classes[i, 3].max():                                            # 518: class 4
            picked.append(i)
    return np.asarray(picked)                                                   # 520


def script_train_indices(all_files, rows, train_idxs0, random):
    """rows[k]: the `fl` the script computes for all_files[k]; random: what the script calls `random`.  The table first, as the
    script builds it -- a path with 'AOI' in it appends its row twice -- then the loop, step by step."""
    table = []
    for k, fn in enumerate(all_files):                                          # 399
        table.append(rows[k])                                                   # 404
        if 'AOI' in fn:                                                         # 405
            table.append(rows[k])
    table = np.asarray(table)                                                   # 407
    picked, with_building, with_damage = [], 0, 0
    for i in train_idxs0:                                                       # 417
        if table[i, :].max():                                                   # 418: any building
            picked.append(i)
            with_building += 1
        if (random.random() > 0.5) and table[i, 1:].max():                      # 421: the draw comes first
            picked.append(i)
            with_damage += 1
    return np.asarray(picked), with_building, with_damage                       # 425


KINDS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 1), (0, 1, 1, 0))       # no building, class 1 only, class 4 only, classes 2 and 3


def class_rows(n, seed):
    """bool [n, 4]: random rows, with the four KINDS forced in at seeded places (n >= 4)"""
    rng = np.random.RandomState(seed)
    fc = rng.random_sample((n, 4)) < 0.35
    for at, kind in zip(rng.permutation(n)[:len(KINDS)], KINDS):
        fc[at] = np.array(kind, dtype=bool)
    return fc


def file_names(n, aoi_at):
    """n paths in the reference's naming; those at `aoi_at` contain 'AOI'"""
    return ["/data/xbd/train/images/%sevent_%08d_pre_disaster.png" % ("AOI_3_" if k in aoi_at else "", k) for k in range(n)]


def table_np(labels):
    """[n, ...] uint8 -> int64 [n, 6]: np.bincount of every file, the bytes above 4 summed into column 5"""
    out = np.zeros((labels.shape[0], 6), dtype=np.int64)
    for f in range(labels.shape[0]):
        b = np.bincount(labels[f].reshape(-1), minlength=256)
        out[f, :5], out[f, 5] = b[:5], b[5:].sum()
    return out


@functools.lru_cache(maxsize=None)
def label_cases(n, hw):
    """name -> (labels uint8 [n, 1, hw], read-only; table_np of it), computed once per shape and shared"""
    rng = np.random.RandomState(1000 * n + hw % 997)
    cases = {"zeros": np.zeros((n, hw), dtype=np.uint8), "threes": np.full((n, hw), 3, dtype=np.uint8),
             "255": np.full((n, hw), 255, dtype=np.uint8), "random 0..4": rng.randint(0, 5, size=(n, hw)).astype(np.uint8),
             "random 0..255": rng.randint(0, 256, size=(n, hw)).astype(np.uint8)}
    for c in END_CLASSES:                       # one byte of class c at either end of every file in a sea of zeros
        a = np.zeros((n, hw), dtype=np.uint8)
        a[:, 0] = a[:, -1] = c
        cases["ends %d" % c] = a
    # neighbouring files of different constant classes: a byte counted for the wrong file shows in two rows
    cases["neighbours"] = np.repeat(np.array([4, 0, 255, 2], dtype=np.uint8)[np.arange(n) % 4][:, None], hw, axis=1)
    out = {}
    for name, a in cases.items():
        a = np.ascontiguousarray(a.reshape(n, 1, hw))
        a.setflags(write=False)
        out[name] = (a, table_np(a))
    return out


# the classes the labels of known_sources hold, file by file: rows of every kind, in an order that puts damage in both parts of
# the seed-0 split
KNOWN_CLASSES = ((), (1,), (4,), (2, 3), (1, 2), (1, 4), (), (3,), (1, 2, 3, 4), (1,), (2,), (1, 3, 4))


def known_sources(H=40, W=52, seed=3):
    """(pre, post [12, H, W, 3], pre_mask [12, H, W], label [12, H, W]) uint8: label k holds exactly KNOWN_CLASSES[k], each class
    as one small rectangle at a seeded place"""
    rng = np.random.RandomState(seed)
    n = len(KNOWN_CLASSES)
    pre = rng.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    post = rng.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    label = np.zeros((n, H, W), dtype=np.uint8)
    for k, classes in enumerate(KNOWN_CLASSES):
        for j, c in enumerate(classes):
            y, x = rng.randint(0, H - 4), 13 * j + rng.randint(0, 9)        # four columns of 13: the rectangles do not overlap
            label[k, y:y + 3, x:x + 4] = c
    return pre, post, ((label > 0) * 255).astype(np.uint8), label

"""CPU: the host side of the input pipeline -- the crop and mosaic specifications, the samplers and a resident epoch's plan -- pinned.

The GPU tests compare what the loaders leave in the step's buffers with `datacoder._crop_resample`, `_crop_gt`, `_mosaic_resample`
and `_mosaic_gt`, so those functions ARE the expected values: a slip in them while they move between modules would move the kernels'
reference with it.  Each case below takes the SHA-256 of the bytes such a function (or a sampler, or one epoch of
`ResidentDataset.__iter__`) returns for inputs built from integer arithmetic, and the test compares it with EXPECTED.

EXPECTED is recorded from the PARENT of the commit that introduced this module (EXPECTED_FROM: the tree in which all of this was
`datacoder.py`'s own), by running `record` below on a checkout of it on the CPU -- never from the code under test.  The cases
therefore use only names both trees have, all reached through `ssdseglib.datacoder`.

  * The specs are float32 arithmetic in the written order, one rounding per operation: their bytes do not depend on the numpy build.
  * The samplers are driven by `StubRng`, a generator whose values come from a fixed arithmetic sequence, so no digest depends on a
    numpy version's bit streams; every case also states how many values its calls consumed.
  * `_augment_rgb` is left out: its `mean` is a float reduction whose order a numpy build may choose (the tolerance tests cover it).

For a later change that moves one of these ON PURPOSE, record the table again from the commit that contains the change:

    python -c "import sys; sys.path[:0] = ['tests', '.']; import conftest, test_cpu_input_spec_pinned as T; T.record(sys.stdout)"

The last two tests are structural: where the moved names live now, and that their modules stay clear of the device.
"""
import ast
import hashlib
import os

import numpy as np
import pytest

H, W = 12, 16
FILL, FILL_CLASS = (7, 200, 31), 3


# ------------------------------------------------------------------------------------------------ inputs
def samples(n):
    """n samples of H x W: pixels and class indices from integer arithmetic"""
    i = np.arange(n * H * W * 3, dtype=np.int64).reshape(n, H, W, 3)
    images = ((i * 37 + (i // 7) * 11 + (i // 48) * 5 + 3) % 256).astype(np.uint8)
    j = np.arange(n * H * W, dtype=np.int64).reshape(n, H, W)
    masks = (((j * 13 + (j // W) * 7) // 3) % 5).astype(np.uint8)
    return images, masks


IDENTITY = (0.0, 0.0, float(W), float(H))
ZOOM_IN = (2.5, 1.25, 9.0, 7.5)             # fractional, inside the image
ZOOM_OUT = (-5.5, -3.25, 28.0, 19.5)        # negative origin, contains the image
RIGHT_EDGE = (6.0, 2.0, 10.0, 8.0)          # x0 + w == W
# every window sees both samples once
WINDOW_SETS = ((IDENTITY, ZOOM_IN), (ZOOM_IN, ZOOM_OUT), (ZOOM_OUT, RIGHT_EDGE), (RIGHT_EDGE, IDENTITY))

# rows (label, xmin, ymin, xmax, ymax) of sample 0; sample 1 has none
ROWS = np.array([
    (1, 1.0, 1.0, 6.0, 5.0),
    (2, 1.5, 3.0, 3.5, 6.0),        # centre x = 2.5: exactly on ZOOM_IN's left edge (inside)
    (3, 10.0, 2.0, 13.0, 4.0),      # centre x = 11.5: exactly on ZOOM_IN's right edge (outside)
    (4, 5.0, 8.25, 9.0, 9.25),      # centre y = 8.75: exactly on ZOOM_IN's lower edge (outside)
    (2, 6.0, 4.0, 6.5, 4.5),        # 0.5 x 0.5: under one pixel through every window but a strong zoom-in
    (1, 0.0, 0.0, 16.0, 12.0),      # the whole image: clipped by every window but the identity and the zoom-out
    (3, 14.5, 9.0, 17.5, 11.5),     # centre x = 16 = W: outside the image, inside the zoom-out only
    (4, 7.0, 3.0, 9.0, 4.4),        # 1.4 high: under one pixel through the zoom-out (12 / 19.5)
], np.float32)


def crop_case():
    D = datacoder()
    images, masks = samples(2)
    gts = [ROWS, np.zeros((0, 5), np.float32)]
    out = []
    for windows in WINDOW_SETS:
        windows = np.array(windows, np.float32)
        img, msk = D._crop_resample(images, masks, windows, FILL, FILL_CLASS)
        out += [img, msk, D._crop_resample_float(images, windows, FILL)]
        for first, second in (gts, gts[::-1]):
            out += D._crop_gt([first, second], windows, H, W)
    only_img, none = D._crop_resample(images, None, np.array(WINDOW_SETS[1], np.float32))       # the default fill, no masks
    assert none is None
    return out + [only_img]


def mosaic_case():
    D = datacoder()
    images, masks = samples(3)
    whole = IDENTITY
    mosaic = D.Mosaic(
        index4=[[0, 0, 0, 0],           # the identity
                [1, 2, 0, 2],           # px == 0: tiles 0 and 2 are empty; source 2 in the two that are left
                [2, 0, 1, 0]],          # source 0 in two tiles
        split=[[W, H], [0, 5], [7, 5]],
        windows=[[whole] * 4,
                 [whole, ZOOM_IN, whole, (-2.0, 1.5, 20.0, 9.0)],
                 [ZOOM_IN, (0.0, 0.0, 16.0, 12.0), ZOOM_OUT, RIGHT_EDGE]])
    gts = [ROWS, np.array([(2, 3.0, 2.0, 9.0, 8.0), (4, 8.0, 6.0, 15.0, 11.0)], np.float32), ROWS[::-1][:5] + np.array([0, 0.25, 0.25, 0.25, 0.25], np.float32)]
    img, msk = D._mosaic_resample(images, masks, mosaic, FILL, FILL_CLASS)
    out = [img, msk]
    counts = []
    for gmax in (3, 64):            # 3 cuts the row lists
        rows = D._mosaic_gt(gts, mosaic, H, W, gmax)
        counts.append([len(r) for r in rows])
        out += rows
    assert max(counts[0]) == 3 and max(counts[1]) > 3, counts        # (the cut was a cut)
    return out


class StubRng:
    """the three methods of numpy's Generator that the samplers use, on a fixed arithmetic sequence: value i is
    ((i * 7919 + 10007) mod 65536) / 65536, exact in float64.  `used`: how many values have been handed out"""

    def __init__(self):
        self.used = 0

    def _take(self, n):
        i = np.arange(self.used, self.used + n, dtype=np.int64)
        self.used += n
        return ((i * 7919 + 10007) % 65536).astype(np.float64) / 65536.0

    def random(self, shape):
        return self._take(int(np.prod(shape))).reshape(shape)

    def uniform(self, lo=0.0, hi=1.0, size=None):
        v = lo + (hi - lo) * self._take(1 if size is None else int(size))
        return float(v[0]) if size is None else v

    def permutation(self, n):
        return np.argsort(self._take(int(n)), kind="stable")


def crop_sampler_case():
    D = datacoder()
    rng, out = StubRng(), []
    out.append(D.random_crop_windows(rng, 9, H, W))
    assert rng.used == 5 * 9
    out.append(D.random_crop_windows(rng, 6, 15, 22, 1.0, (0.02, 40.0), (0.1, 10.0)))        # both clamps
    out.append(D.random_crop_windows(rng, 4, H, W, probability=0.0))
    assert rng.used == 5 * (9 + 6 + 4)
    return out


def mosaic_sampler_case():
    D = datacoder()
    rng, out = StubRng(), []
    for args in ((9, H, W), (6, 15, 22, 1.0, (0.0, 1.0), (0.01, 40.0)), (4, H, W, 0.0)):
        m = D.random_mosaic(rng, *args)
        out += [m.index4, m.split, m.windows]
    assert rng.used == 18 * (9 + 6 + 4)
    return out


def epoch_plan_case():
    D = datacoder()
    rng, out = StubRng(), []
    for args, used in (((7, 3, True, True, True, False), 7 + 7 + 4 * 3), ((7, 3, False, False, False, True), 0),
                       ((8, 4, True, False, True, True), 8 + 4 * 2), ((5, 2, False, True, False, False), 5)):
        before = rng.used
        plan = D._epoch_plan(rng, *args)
        assert rng.used - before == used, args
        out.append(len(plan))
        for index, flip, draws in plan:
            out += [index, flip, None if draws is None else np.array(draws, np.float64)]
    return out


def _batch_fields(batch):
    draws = None if batch.rgb_draws is None else np.array(batch.rgb_draws, np.float64)
    fill = None if batch.crop_fill is None else np.array(batch.crop_fill, np.int64)
    mosaic_fill = None if batch.mosaic_fill is None else np.array(batch.mosaic_fill, np.int64)
    mosaic = [None] * 3 if batch.mosaic is None else [batch.mosaic.index4, batch.mosaic.split, batch.mosaic.windows]
    return [batch.index, batch.flip, draws, batch.crop_windows, fill, mosaic_fill] + mosaic


def _planned_epochs(used_per_epoch, **options):
    """two epochs of a ResidentDataset of 7 samples in batches of 3 that holds no sample: nothing is written, so no device is touched"""
    D = datacoder()
    anchors = np.array([1.0, 2.0], np.float32)
    encoder = D.DataEncoderDecoder(5, (H, W), anchors, anchors, anchors + 4, anchors + 4, augmentation_horizontal_flip=True)
    ds = D.ResidentDataset(encoder, capacity=7, batch_size=3, rgb_augmentation=True, **options)
    ds.num_samples, ds._rng = 7, StubRng()
    out = []
    for epoch in (1, 2):
        batches = list(ds)
        assert [len(b) for b in batches] == [3, 3, 1] and ds._rng.used == epoch * used_per_epoch
        for b in batches:
            out += _batch_fields(b)
    assert ds.images is None and ds.ctx is None
    return out


PLAN = 7 + 7 + 4 * 3        # the permutation, the flips, one colour draw set per batch


def resident_plain_case():
    return _planned_epochs(PLAN)


def resident_crop_case():       # the windows come after the whole plan, batch by batch
    return _planned_epochs(PLAN + 5 * 7, random_crop={"probability": 0.8, "scale": (0.4, 2.5), "fill": FILL, "fill_class": FILL_CLASS})


def resident_mosaic_case():     # one draw for the epoch's mosaics, after the whole plan
    return _planned_epochs(PLAN + 18 * 7, mosaic={"probability": 0.7, "center": (0.2, 0.8), "fill": FILL, "fill_class": FILL_CLASS})


CASES = {"crop spec": crop_case, "mosaic spec": mosaic_case, "random_crop_windows": crop_sampler_case, "random_mosaic": mosaic_sampler_case,
         "_epoch_plan": epoch_plan_case, "resident epoch, plain": resident_plain_case, "resident epoch, random_crop": resident_crop_case,
         "resident epoch, mosaic": resident_mosaic_case}


# ------------------------------------------------------------------------------------------------ digests
def datacoder():
    from ssdseglib import datacoder as D
    return D


def digest(items):
    """SHA-256 over the items in order: an array as its dtype, shape and bytes, an int or None as its repr; and how many there were"""
    sha = hashlib.sha256()
    for x in items:
        if isinstance(x, np.ndarray):
            sha.update(f"{x.dtype.str}{x.shape}".encode())
            sha.update(np.ascontiguousarray(x).tobytes())
        else:
            assert x is None or isinstance(x, int), type(x)
            sha.update(repr(x).encode())
    return sha.hexdigest(), len(items)


def record(out):
    """prints the table of this tree (for EXPECTED: run it on the commit the table is to be taken from, see the module docstring)"""
    out.write("EXPECTED = {\n")
    for name, case in CASES.items():
        out.write(f"    {name!r}: {digest(case())!r},\n")
    out.write("}\n")


@pytest.mark.parametrize("name", list(CASES))
def test_input_specs_samplers_and_plans_are_pinned(name):
    assert digest(CASES[name]()) == EXPECTED[name], name


def test_expected_table_is_not_empty():
    assert set(EXPECTED) == set(CASES)
    assert all(len(sha) == 64 and items >= 3 for sha, items in EXPECTED.values())


# Recorded with `record` above on the CPU from a checkout of the commit named here (the parent of the commit that introduced this
# module).  {case: (SHA-256 of its items, their number)}
EXPECTED_FROM = "e54f1d62be0d8455553b5e42f6d89602285257b3"
EXPECTED = {
    'crop spec': ('a40497091c680eb8bc13e98fe0eaafc93018cf211fd03ed1e4fb8061b40e6509', 29),
    'mosaic spec': ('74d863f4a14c032d32c42f3f01c405fa77c384a9172feea04e8cfee287cbb820', 8),
    'random_crop_windows': ('6a8c4ec46bb3d4458bcbdf157782e4079b6ec33185fdbd9a55236275f35bac49', 3),
    'random_mosaic': ('fdae9a20a3b226fc0a5b2f9f0fce22ba065e7ed72f8a92831e334cc7217af986', 9),
    '_epoch_plan': ('ab402a954003b236b80c5b8f445c1285f8b20591dbfbf96eda6b030be845adfe', 34),
    'resident epoch, plain': ('f31cba6c0bde6094aadc2453bddafe1bef72fbd81abda02566f53440251d3ac3', 54),
    'resident epoch, random_crop': ('788f707cd4ac443281d61d848d5ac2c0586b10325c88c7e68ac1c1c685be65b8', 54),
    'resident epoch, mosaic': ('37d580075f53ca717d0732b4c9e15129d3c23dc5028a0b9c9bc84452aee19c13', 54),
}


# ------------------------------------------------------------------------------------------------ where the names live
HOMES = {
    "_batches": ("Mosaic", "CompactBatch", "ResidentBatch"),
    "_resident": ("ResidentDataset",),
    "_samplers": ("random_crop_windows", "random_mosaic", "_epoch_plan"),
    "_augment_spec": ("_crop_resample", "_crop_resample_float", "_crop_gt", "_mosaic_resample", "_mosaic_gt", "_augment_rgb", "_rgb_to_hsv",
                      "_hsv_to_rgb"),
}
# what a module may import at its top level, besides the standard library and numpy: its siblings below it
MAY_IMPORT = {"_batches": set(), "_augment_spec": {"_batches"}, "_samplers": {"_batches"}, "_resident": {"_batches", "_samplers"}}


def test_reexported_names_are_the_objects_of_their_new_homes():
    import importlib
    D = datacoder()
    for module, names in HOMES.items():
        home = importlib.import_module("ssdseglib." + module)
        for name in names:
            assert getattr(D, name) is getattr(home, name), (module, name)
            assert getattr(home, name).__module__ == "ssdseglib." + module, (module, name)
    # the reference-shaped surface and its three streams stay datacoder's own
    for name in ("DataEncoderDecoder", "read_image", "augmentation_rgb_channels", "augmentation_random_crop", "augmentation_mosaic", "_draw_rgb"):
        assert getattr(D, name).__module__ == "ssdseglib.datacoder", name
    for name in ("_aug_rng", "_crop_rng", "_mosaic_rng"):
        assert isinstance(vars(D)[name], np.random.Generator), name


def _imports(tree, top_level_only):
    """the package-relative modules (and numpy-or-stdlib ones, by their first name) that a module's import statements name"""
    nodes = tree.body if top_level_only else list(ast.walk(tree))
    relative, absolute = set(), set()
    for node in nodes:
        if isinstance(node, ast.Import):
            absolute |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            if node.level == 0:
                absolute.add(node.module.split(".")[0])
            else:
                relative |= {node.module.split(".")[0]} if node.module else {a.name for a in node.names}
    return relative, absolute


@pytest.mark.parametrize("module", list(MAY_IMPORT))
def test_new_modules_stay_clear_of_the_device(module):
    """no import of _hip, _engine or _loaders when the module is loaded (the package's __init__ loads those through other modules, so
    the module's own import statements are what is read); the spec and sampler modules name them nowhere, and the dataset's device
    context stays a lazy import inside a method"""
    import ssdseglib
    path = os.path.join(os.path.dirname(ssdseglib.__file__), module + ".py")
    tree = ast.parse(open(path).read())
    relative, absolute = _imports(tree, top_level_only=True)
    assert relative <= MAY_IMPORT[module], relative
    assert absolute <= {"numpy", "typing", "__future__"}, absolute
    anywhere, _ = _imports(tree, top_level_only=False)
    assert not anywhere & {"_hip", "_loaders"}, anywhere
    assert ("_engine" in anywhere) == (module == "_resident"), anywhere

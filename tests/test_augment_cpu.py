"""The declared colour augmentation without a GPU (include/cad/cad.h, cad_sample / cad_aug_config: saturation, hue,
gamma — keys every shipped config declares and the reference's augmentSample never applies).

Sampler: the three extra draws come after augmentSample's six from the same std::mt19937, bit-identical to the
restatement (tests/augment_restatement.py over oracle.StdMt19937Draws); with the three off the stream is the
reference's.  cad_color_matrix against the float64 restatement (1 fp32 ulp: libm's and numpy's cos / sin may
differ in the last bit of the double), its exact identities, and the refusal of every bad config value by name.
build/train: data.augmentation.mode / --augmentation, judged before any GPU call; the reference mode's plan does
not depend on the declared keys."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import yaml

import augment_restatement as R
from conftest import ROOT

PKG = os.path.join(ROOT, "camera-aware-neural-networks-for-few-view-depth-estimation_amd")
TRAIN = os.path.join(ROOT, "build", "train")

BASE = dict(enable_random_crop=1, crop_scale_min=0.7, crop_scale_max=1.0, enable_horizontal_flip=1,
            horizontal_flip_prob=0.5, enable_color_jitter=1, brightness_delta=0.2, contrast_delta=0.2)
OFF = dict(saturation_delta=0.0, hue_delta=0.0, enable_random_gamma=0, gamma_min=0.0, gamma_max=0.0)
CONFIGS = {
    "all": dict(BASE, saturation_delta=0.3, hue_delta=0.1, enable_random_gamma=1, gamma_min=0.7, gamma_max=1.3),
    "saturation": dict(BASE, **dict(OFF, saturation_delta=0.2)),
    "hue": dict(BASE, **dict(OFF, hue_delta=0.1)),
    "gamma": dict(BASE, **dict(OFF, enable_random_gamma=1, gamma_min=0.8, gamma_max=1.2)),
    # colour jitter off: saturation / hue are not drawn whatever their deltas; crop off as well
    "gamma_no_jitter": dict(BASE, enable_random_crop=0, enable_color_jitter=0, saturation_delta=0.2, hue_delta=0.1,
                            enable_random_gamma=1, gamma_min=1.0, gamma_max=1.0),
    "off": dict(BASE, **OFF),
}


def _f32(v):
    return C.c_float(v).value


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("seed,H,W", [(42, 480, 640), (7, 48, 64), (12345, 97, 131)])
def test_sampler_matches_restatement(cad, oracle, name, seed, H, W):
    from cad_amd import _abi
    cfg = CONFIGS[name]
    lib = cad.load_library()
    h = C.c_void_p()
    conf = _abi.AugConfig(**cfg)
    assert lib.cad_aug_sampler_create(C.byref(conf), seed, C.byref(h)) == 0, lib.cad_last_error()
    ref = R.DeclaredDraws(seed, cfg)
    plain = oracle.StdMt19937Draws(seed, cfg) if name == "off" else None
    try:
        for _ in range(64):
            s = _abi.Sample()
            assert lib.cad_aug_sampler_draw(h, H, W, C.byref(s)) == 0
            r = ref.draw(H, W)
            assert (s.aug, s.crop, s.flip, s.jitter) == (1, r["crop"], r["flip"], r["jitter"])
            if r["crop"]:
                assert (s.crop_scale, s.crop_x, s.crop_y) == (_f32(r["crop_scale"]), r["crop_x"], r["crop_y"])
            if r["jitter"]:
                assert (s.brightness, s.contrast) == (_f32(r["brightness"]), _f32(r["contrast"]))
            assert (s.color, s.gamma_on) == (r["color"], r["gamma_on"])
            assert (s.saturation, s.hue, s.gamma) == (_f32(r["saturation"]), _f32(r["hue"]), _f32(r["gamma"]))
            if r["color"] and cfg["saturation_delta"] > 0:
                assert 1 - _f32(cfg["saturation_delta"]) - 1e-6 <= s.saturation <= 1 + _f32(cfg["saturation_delta"]) + 1e-6
            if plain is not None:   # all off: the engine advances exactly as the reference's
                q = plain.draw(H, W)
                assert (s.color, s.gamma_on, s.saturation, s.hue, s.gamma) == (0, 0, 1.0, 0.0, 1.0)
                assert all(_f32(r[k]) == _f32(q[k]) for k in q)
    finally:
        lib.cad_aug_sampler_destroy(h)
    expect = {"all": (1, 1), "saturation": (1, 0), "hue": (1, 0), "gamma": (0, 1), "gamma_no_jitter": (0, 1), "off": (0, 0)}
    assert (r["color"], r["gamma_on"]) == expect[name]


def test_python_sampler_returns_new_fields(cad):
    s = cad.AugSampler(42, **CONFIGS["all"])
    r = R.DeclaredDraws(42, CONFIGS["all"])
    for _ in range(4):
        d, q = s.draw(48, 64), r.draw(48, 64)
        assert {k: _f32(v) for k, v in q.items()} == {k: d[k] for k in q}
    d = cad.AugSampler(42).draw(48, 64)   # defaults: the new stages are off
    assert (d["color"], d["gamma_on"]) == (0, 0)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


def test_color_matrix(cad):
    rng = np.random.default_rng(0)
    pairs = [(1.0, 0.0), (0.0, 0.0), (1.3, 0.1), (0.7, -0.1), (1.0, 0.25), (1.0, 0.5), (0.5, -0.5), (1.5, 0.37)]
    pairs += [(rng.uniform(0, 2), rng.uniform(-0.5, 0.5)) for _ in range(200)]
    for s, hue in pairs:
        M, ref = cad.color_matrix(s, hue), R.color_matrix(s, hue)
        assert M.dtype == np.float32 and M.shape == (3, 3)
        assert np.all(np.abs(M.astype(np.float64) - ref) <= np.spacing(np.abs(ref))), (s, hue)   # 1 ulp per entry
        rows = M.astype(np.float64).sum(1)
        assert np.all(np.abs(rows - 1.0) <= 2 * 2.0 ** -23), (s, hue, rows)
    assert np.array_equal(cad.color_matrix(1.0, 0.0), np.eye(3, dtype=np.float32))
    assert np.array_equal(cad.color_matrix(0.0, 0.0), np.tile(R.LUMA, (3, 1)))
    assert np.array_equal(cad.color_matrix(0.0, 0.3), np.tile(R.LUMA, (3, 1)))   # no chroma left to rotate
    # theta = 0: the blend with the luma grey, s I + (1 - s) luma rows
    s = 0.75
    blend = s * np.eye(3) + (1 - s) * np.tile(R.T[0], (3, 1))
    assert np.abs(cad.color_matrix(s, 0.0) - blend).max() <= 2.0 ** -23
    # the row abs-sums behind the tests' tolerances
    norm = lambda s, h: np.abs(cad.color_matrix(s, h).astype(np.float64)).sum(1).max()
    assert max(norm(s, h) for s in (0.7, 1.0, 1.3) for h in np.linspace(-0.1, 0.1, 21)) <= 2.95
    lib = cad.load_library()
    out = (C.c_float * 9)()
    assert lib.cad_color_matrix(float("nan"), 0.0, out) != 0 and b"finite" in lib.cad_last_error()


@pytest.mark.parametrize("field,kw", [
    ("saturation_delta", dict(saturation_delta=-0.1)),
    ("saturation_delta", dict(saturation_delta=1.5)),
    ("saturation_delta", dict(saturation_delta=float("nan"))),
    ("hue_delta", dict(hue_delta=0.6)),
    ("hue_delta", dict(hue_delta=-0.01)),
    ("gamma_min", dict(enable_random_gamma=1, gamma_min=0.0, gamma_max=1.2)),
    ("gamma_min", dict(enable_random_gamma=1, gamma_min=-0.5, gamma_max=1.2)),
    ("gamma_min", dict(enable_random_gamma=1, gamma_min=float("nan"), gamma_max=1.2)),
    ("gamma_max", dict(enable_random_gamma=1, gamma_min=1.2, gamma_max=0.8)),
    ("gamma_max", dict(enable_random_gamma=1, gamma_min=0.8, gamma_max=float("inf"))),
])
def test_sampler_refuses_bad_values(cad, field, kw):
    from cad_amd import _abi
    lib = cad.load_library()
    h = C.c_void_p()
    conf = _abi.AugConfig(**kw)
    assert lib.cad_aug_sampler_create(C.byref(conf), 1, C.byref(h)) != 0
    assert field.encode() in lib.cad_last_error()
    with pytest.raises(cad.CadError, match=field):
        cad.AugSampler(1, **kw)


def test_gamma_range_ignored_when_gamma_is_off(cad):
    cad.AugSampler(1, enable_random_gamma=0, gamma_min=0.0, gamma_max=-1.0).draw(48, 64)


# ---------------------------------------------------------------- build/train
@pytest.fixture(scope="module")
def train_bin():
    subprocess.run(["make", "-C", PKG, "-o", "libcad_hip.so", "train"], check=True, capture_output=True)
    return TRAIN


def _cfg(tmp_path, name="a.yaml", **aug):
    cfg = {"data": {"dataset_name": "sunrgbd", "manifest_path": "./manifest.json", "input_height": 48, "input_width": 64,
                    "augmentation": dict({"random_crop": True, "horizontal_flip": True, "color_jitter": True,
                                          "brightness": 0.2, "contrast": 0.2}, **aug)},
           "model": {"init_features": 16}, "training": {"batch_size": 2, "num_epochs": 1}}
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return p


def _manifest(tmp_path, n=3):
    """A manifest whose samples have an intrinsics.txt (all a --dry-run looks at)."""
    images = []
    for k in range(n):
        rel = f"./data/s{k}"
        (tmp_path / rel).mkdir(parents=True)
        (tmp_path / rel / "intrinsics.txt").write_text("518.8 0 325.5\n0 519.4 253.7\n0 0 1\n")
        images.append({"path": rel, "sensor_type": "kv1", "valid": True})
    (tmp_path / "manifest.json").write_text(json.dumps({"dataset": "SUN RGB-D V1", "images": images}))


def _dry(train_bin, tmp_path, p, *flags):
    return subprocess.run([train_bin, "-c", str(p), "--dry-run", *flags], capture_output=True, text=True, timeout=60,
                          cwd=tmp_path)


DECLARED = dict(saturation=0.3, hue=0.1, random_gamma=True, gamma_range=[0.7, 1.3])


def test_cli_declared_dry_run_states_the_ranges(train_bin, tmp_path):
    _manifest(tmp_path)
    r = _dry(train_bin, tmp_path, _cfg(tmp_path, mode="declared", **DECLARED))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and json.loads(lines[0])["steps_per_epoch"] == 2
    assert lines[1] == ("Augmentation (declared): saturation [0.699999988, 1.29999995], hue [-0.100000001, 0.100000001], "
                        "gamma [0.699999988, 1.29999995]")
    # the flag overrides the config either way
    r = _dry(train_bin, tmp_path, _cfg(tmp_path, mode="declared", **DECLARED), "--augmentation", "reference")
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == 1
    r = _dry(train_bin, tmp_path, _cfg(tmp_path, **dict(DECLARED, random_gamma=False)), "--augmentation=declared")
    assert r.returncode == 0 and r.stdout.strip().splitlines()[1].endswith("hue [-0.100000001, 0.100000001], gamma off")


@pytest.mark.parametrize("aug,flags,msg", [
    (dict(DECLARED, mode="declared", gamma_range=[1.3, 0.7]), (), "Error: data.augmentation.gamma_range"),
    (dict(DECLARED, mode="declared", gamma_range=[0.0, 1.0]), (), "Error: data.augmentation.gamma_range"),
    (dict(DECLARED, mode="declared", gamma_range=[0.8]), (), "Error: data.augmentation.gamma_range"),
    (dict(DECLARED, gamma_range=[-1.0, 1.0]), ("--augmentation", "declared"), "Error: data.augmentation.gamma_range"),
    (dict(DECLARED, mode="declared", saturation=1.5), (), "Error: data.augmentation.saturation"),
    (dict(DECLARED, mode="declared", hue=0.75), (), "Error: data.augmentation.hue"),
    (dict(DECLARED, mode="everything"), (), "Error: data.augmentation.mode 'everything'"),
    (dict(DECLARED), ("--augmentation", "both"), "Error: --augmentation 'both'"),
])
def test_cli_refuses_bad_declared_values(train_bin, tmp_path, aug, flags, msg):
    _manifest(tmp_path)
    r = _dry(train_bin, tmp_path, _cfg(tmp_path, **aug), *flags)
    assert r.returncode == 1 and r.stderr.startswith(msg), (r.returncode, r.stderr)
    assert r.stdout == ""


def test_cli_reference_plan_ignores_the_declared_keys(train_bin, tmp_path):
    """The reference mode's --dry-run output with and without the four keys — whatever they hold — is the same
    text.  One field is masked: "id_hash" is the hash of random bytes a dry run draws in place of the
    communicator id (train_main.cpp, exchange_id), different in any two runs by construction."""
    _manifest(tmp_path)
    mask = lambda t: re.sub(r'"id_hash": \d+', '"id_hash": 0', t)
    outs = []
    for k, aug in enumerate([{}, DECLARED, dict(saturation=7.0, hue=-3.0, random_gamma=True, gamma_range=[2.0, -1.0]),
                             dict(DECLARED, mode="reference")]):
        r = _dry(train_bin, tmp_path, _cfg(tmp_path, **aug))
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert '"id_hash": ' in r.stdout
        outs.append(mask(r.stdout))
    assert outs[0] == outs[1] == outs[2] == outs[3]
    assert "Augmentation" not in outs[0]


def test_shipped_augment_config(train_bin, tmp_path):
    """configs/train_config_augment.yaml declares the mode and the production ranges."""
    _manifest(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_config_augment.yaml")))
    assert cfg["data"]["augmentation"]["mode"] == "declared"
    cfg["data"]["manifest_path"] = "./manifest.json"
    p = tmp_path / "shipped.yaml"
    p.write_text(yaml.safe_dump(cfg))
    r = _dry(train_bin, tmp_path, p)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("Augmentation (declared): saturation [")

"""The pieces the raw data routes share (leftrefill_amd/rawbatch.py) on the CPU: the arena packer, and that every raw-capable dataset
names a collate function and a device prep that agree with the plans it emits -- over the trees the dataset tests already build."""
import numpy as np
import pytest
import torch

import leftrefill_amd.dropin as dropin

dropin.install()
from dataloaders.raw_pairs import TestInpaintingDataset as RawTestInpaintingDataset  # noqa: E402
from leftrefill_amd import dataprep, nvsprep, rawbatch  # noqa: E402
import test_nvsdata_cpu as TN  # noqa: E402
import test_pairdata_cpu as TP  # noqa: E402
from test_dataprep_cpu import _train, data  # noqa: E402, F401  (`data` is that module's fixture)


@pytest.mark.parametrize("align,offsets,length", [(1, [0, 5, 21], 64), (16, [0, 16, 32], 80)])
def test_arena_offsets_zero_gaps_and_tail(align, offsets, length):
    rng = np.random.RandomState(align)
    sources = [rng.randint(1, 256, n, dtype=np.uint8) for n in (5, 16, 33)]      # no zero byte: every zero below is the arena's
    sources[1] = sources[1].reshape(4, 4).T                                        # not C-contiguous: copied as if it were
    arena = rawbatch.Arena(align)
    assert [arena.add(s) for s in sources] == offsets
    got = arena.tensor(False)
    assert got.dtype == torch.uint8 and got.numel() == length and length % 16 == 0 and not got.is_pinned()
    want = np.zeros(length, np.uint8)
    for off, s in zip(offsets, sources):
        want[off:off + s.size] = np.ascontiguousarray(s).reshape(-1)
    assert got.numpy().tobytes() == want.tobytes()
    assert int((got.numpy() == 0).sum()) == length - 54      # gaps and tail, nothing else


def test_an_empty_arena_is_16_zero_bytes():
    for align in (1, 16):
        assert rawbatch.Arena(align).tensor(False).tolist() == [0] * 16


def test_a_source_that_is_not_uint8_is_refused():
    arena = rawbatch.Arena(1)
    for bad in (np.zeros(4, np.int8), np.zeros((2, 2), np.float32), np.zeros(3, bool)):
        with pytest.raises(AssertionError, match="uint8"):
            arena.add(bad)
    assert arena.end == 0 and arena.tensor(False).numel() == 16


def test_table_tensor_and_default_pin():
    jobs = np.zeros(3, dtype=nvsprep.JOB_DTYPE)
    jobs["k"] = [1, 2, 3]
    table = rawbatch.table_tensor(jobs, False)
    assert table.dtype == torch.uint8 and table.numpy().tobytes() == jobs.tobytes() and table.numel() == 3 * 120
    assert rawbatch.default_pin(False) is False and rawbatch.default_pin(True) is True
    assert rawbatch.default_pin(None) is torch.cuda.is_available()      # the tests' process is no loader worker


def _raw_datasets(data, tmp_path_factory):      # noqa: F811
    """(dataset with raw=True, its collate function, its prep class, the numpy statement of its plans), one per raw-capable class."""
    pairs, nvs = TP.Fixture(tmp_path_factory.mktemp("pair_tree")), TN.Fixture(tmp_path_factory.mktemp("nvs_tree"))
    out = [(_train(data, raw=True), dataprep.collate_raw, dataprep.DevicePrep, dataprep.run_plan_numpy),
           (RawTestInpaintingDataset(pairs.root + "/val", img_size=TP.S, mask_path=pairs.root + "/val_masks", raw=True),
            dataprep.collate_raw, dataprep.DevicePrep, dataprep.run_plan_numpy)]
    for name, cls in (("val", TP.InpaintingCrossViewDataset), ("mv_plain_v4", TP.InpaintingMultiViewDataset),
                      ("mv_concat_v3", TP.InpaintingMultiViewDataset)):
        kwargs = pairs.spec["mv_settings" if name.startswith("mv") else "settings"][name][0]
        out.append((cls(**TP.G.resolve(kwargs, pairs.root), raw=True), dataprep.collate_raw, dataprep.DevicePrep, dataprep.run_plan_numpy))
    kwargs = nvs.spec["settings"]["train_enlarge"][0]
    out.append((TN.NVS_OBJDataset(**TN.G.resolve(kwargs, nvs.root), raw=True), nvsprep.collate_nvs_raw, nvsprep.NVSDevicePrep,
                nvsprep.run_nvs_plan_numpy))
    return out


def test_every_raw_dataset_names_its_collate_function_and_a_prep_that_fits_its_plans(data, tmp_path_factory):      # noqa: F811
    from torch.utils.data import DataLoader
    seen = set()
    for ds, collate, prep_cls, run in _raw_datasets(data, tmp_path_factory):
        np.random.seed(5)
        item = ds[0]
        plan, raw = item
        assert type(ds).collate_raw is collate and ds.collate_raw is collate, type(ds)
        prep = ds.device_prep("cpu")
        assert type(prep) is prep_cls and prep.device == torch.device("cpu") and ds.device_prep().device.type == "cuda"
        batch = ds.collate_raw([item, item], pin=False)
        canvas = np.asarray(run(plan, raw)["image"])      # [S, T S, 3], or [V, S, T S, 3]
        S, T = plan["img_size"], prep.tiles
        assert prep.img_size == S == ds.img_size == batch["img_size"] and canvas.shape[-3:] == (S, T * S, 3), (type(ds), canvas.shape, T)
        if collate is dataprep.collate_raw:
            assert batch["tiles"] == T == len(dataprep.plan_canvases(plan)[0]) and len(dataprep.job_table(batch)) == 2 * batch.get("views", 1) * T
        seen.add((type(ds).__name__, T))
        # the loader helper: the plain DataLoader, the raw-collating one, and that one behind the dataset's prep
        plain = rawbatch.loader(ds, False, "cpu", batch_size=2)
        inner, chained = rawbatch.loader(ds, True, batch_size=2), rawbatch.loader(ds, True, "cpu", batch_size=2, shuffle=False)
        assert type(plain) is DataLoader and plain.collate_fn is not collate and not plain.pin_memory
        assert type(inner) is DataLoader and inner.collate_fn is collate and inner.pin_memory and inner.batch_size == 2
        assert type(chained) is rawbatch.DevicePrepLoader is dataprep.DevicePrepLoader and type(chained.prep) is prep_cls
        assert chained.loader.collate_fn is collate and chained.dataset is ds and len(chained) == len(inner) == len(plain)
        assert (chained.prep.img_size, chained.prep.tiles, chained.prep.device) == (S, T, torch.device("cpu"))
    assert seen == {("InpaintingDataset", 1), ("TestInpaintingDataset", 2), ("InpaintingCrossViewDataset", 2),
                    ("InpaintingMultiViewDataset", 1), ("InpaintingMultiViewDataset", 2), ("NVS_OBJDataset", 2)}


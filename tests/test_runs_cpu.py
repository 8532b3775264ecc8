"""CPU: the loop control of the recognition and part-seg runs (ppt_amd/runs.py) and the argument parsing of their commands."""
import pytest

from ppt_amd import runs


@pytest.mark.parametrize("n_batches, data_ratio, processed", [(10, 0.3, 4), (10, 0.7, 8), (4, 0.5, 3), (5, 1.0, 5), (329, 0.3, 99),
                                                               (1, 0.05, 1)])
def test_epoch_plan_follows_the_break_rule(n_batches, data_ratio, processed):
    """main_cls.py:173-174: `if data_iter > len(train_loader) * args.data_ratio: break`, the product an unrounded Python float"""
    plan = runs.epoch_plan(n_batches, 0, data_ratio)
    assert [p[0] for p in plan] == list(range(processed))
    want = [i for i in range(n_batches) if not i > n_batches * data_ratio]          # (every skipped batch follows every kept one)
    assert [p[0] for p in plan] == want
    assert all(p[2] for p in plan) and [p[1] for p in plan] == list(range(processed))      # update_freq 1: all metered, index = batch


def test_epoch_plan_schedule_index_and_metered_steps():
    plan = runs.epoch_plan(5, 1, 1.0, 2)                       # main_cls.py:160, :181-183, :209
    assert [p[0] for p in plan] == [0, 1, 2, 3, 4]
    assert [p[1] for p in plan] == [2, 2, 3, 3, 4]
    assert [p[2] for p in plan] == [False, True, False, True, False]
    # every batch is a step of its own: update_freq is no gradient accumulation, the plan has one entry per batch
    assert len(runs.epoch_plan(8, 0, 1.0, 4)) == 8 and [p[2] for p in runs.epoch_plan(8, 0, 1.0, 4)].count(True) == 2
    # data_ratio and update_freq together: 10 * 0.3 -> batches 0..3, index data_iter // 3 on top of 3 * epoch
    assert runs.epoch_plan(10, 2, 0.3, 3) == [(0, 6, False), (1, 6, False), (2, 6, True), (3, 7, False)]
    assert runs.epoch_plan(0, 0) == []
    with pytest.raises(ValueError):
        runs.epoch_plan(4, 0, 1.0, 0)


def test_schedule_index_is_clamped_in_the_last_epoch():
    """n_batches % update_freq != 0: the schedule has epochs * (5 // 2) = 4 entries and the last batch of the last epoch asks for
    entry 4, where the reference raises IndexError; here it reads the last entry"""
    epochs, n_batches, update_freq = 2, 5, 2
    length = epochs * (n_batches // update_freq)
    plan = runs.epoch_plan(n_batches, epochs - 1, 1.0, update_freq)
    assert [p[1] for p in plan] == [2, 2, 3, 3, 4] and plan[-1][1] == length
    assert [runs.clamp_index(p[1], length) for p in plan] == [2, 2, 3, 3, 3]
    assert [runs.clamp_index(p[1], length) for p in runs.epoch_plan(n_batches, 0, 1.0, update_freq)] == [0, 0, 1, 1, 2]


def test_meter_average():
    assert runs.meter_average(7.9, 4) == 1.975                 # utils/utils.py:337
    got = runs.meter_average(7.9, 4, world_sums=[[3.6, 2], [4.3, 2]])
    assert got == 7 / 4                                        # :346: the all-reduced sum truncated to an integer
    assert runs.meter_average(3.6, 2, world_sums=[[3.6, 2]]) == 3 / 2


def test_recognition_command_arguments():
    """python -m ppt_amd.recognition: the reference's flag names with parser.py's defaults; parsing touches no GPU"""
    from ppt_amd import recognition
    a = recognition.parse_args(["--train", "tr.npz", "--test", "te.npz"])
    assert (a.model, a.dataset_name, a.head_type, a.data_ratio, a.update_freq, a.optim) == ("ULIP_PN_SSG", "modelnet40", 0, 1.0, 1, "adamw")
    assert (a.epochs, a.batch_size, a.npoints, a.lr, a.lr_start, a.lr_end, a.warmup_epochs) == (250, 64, 8192, 3e-3, 1e-6, 1e-5, 1)
    assert (a.wd, a.betas, a.eps, a.label_smoothing, a.print_freq, a.seed) == (0.1, (0.9, 0.98), 1e-8, 0.3, 10, 0)
    assert (a.use_height, a.ulip2, a.class_name_position, a.num_learnable_prompt_tokens) == (False, False, "end", 32)
    assert (a.task, a.recipe, a.rank, a.world_size, a.output_dir) == ("cls", "modelnet", 0, 1, "outputs")
    a = recognition.parse_args(["--train", "a", "--test", "b", "--model", "ULIP_PN_NEXT", "--use_height", "--ulip2", "--head_type", "2",
                                "--data_ratio", "0.3", "--update_freq", "2", "--optim", "sgd", "--dataset_name", "scanobjectnn",
                                "--betas", "0.8", "0.9"])
    assert (a.model, a.use_height, a.ulip2, a.head_type, a.data_ratio, a.update_freq, a.optim) == ("ULIP_PN_NEXT", True, True, 2, 0.3, 2, "sgd")
    assert a.recipe == "scanobjectnn" and a.betas == (0.8, 0.9)
    assert recognition.parse_args(["--train", "a", "--test", "b", "--dataset_name", "shapenet55"]).recipe == "shapenet55"
    with pytest.raises(SystemExit):
        recognition.parse_args(["--train", "a", "--test", "b", "--optim", "lion"])
    for k, v in recognition.DEFAULTS.items():                  # run_cls's own defaults are the command's
        if k not in ("recipe", "rank", "world_size", "output_dir", "gpu"):
            assert getattr(recognition.parse_args(["--train", "a", "--test", "b"]), k) == v, k


def test_partseg_command_arguments():
    from ppt_amd import partseg
    a = partseg.parse_args(["--train", "tr.npz", "--test", "va.npz", "--epochs", "3", "--optim", "adam", "--data_ratio", "0.5"])
    assert (a.model, a.dataset_name, a.task, a.recipe, a.epochs, a.optim, a.data_ratio) == \
        ("ULIP_PointBERT_partseg", "shapenetpart", "partseg", "shapenetpart", 3, "adam", 0.5)
    c2p = a.category2part
    assert len(c2p) == 16 and sum(len(v) for v in c2p.values()) == 50
    assert c2p["Airplane"] == [0, 1, 2, 3] and c2p["Motorbike"] == [30, 31, 32, 33, 34, 35] and c2p["Table"] == [47, 48, 49]
    assert [p for v in c2p.values() for p in v] == list(range(50))

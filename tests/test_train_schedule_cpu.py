"""stmask_amd.train.lr_at and autoscale against the reference's formulas (train.py:293-302 and :88-96), the expected values written out."""
from stmask_amd.train import autoscale, lr_at

LR, GAMMA, STEPS, UNTIL, INIT = 1e-3, 0.1, (150000, 200000), 500, 1e-4       # the STMask configs (config.py:403-415, :625)


def at(it, steps=STEPS, until=UNTIL):
    return lr_at(it, LR, GAMMA, steps, until, INIT)


def test_warm_up_ramp():
    assert at(0) == (1e-3 - 1e-4) * (0 / 500) + 1e-4 == 1e-4
    assert at(250) == (1e-3 - 1e-4) * (250 / 500) + 1e-4
    assert abs(at(250) - 5.5e-4) < 1e-18
    assert at(500) == (1e-3 - 1e-4) * (500 / 500) + 1e-4
    # after the warm-up the optimizer keeps what iteration 500 set, in the loop's arithmetic (within an ulp of lr)
    assert at(501) == at(149999) == at(500) and abs(at(501) - 1e-3) < 1e-18


def test_steps():
    assert at(149999) == at(500)
    assert at(150000) == 1e-3 * (0.1 ** 1)
    assert at(199999) == 1e-3 * (0.1 ** 1)
    assert at(200000) == 1e-3 * (0.1 ** 2)
    assert at(10 ** 6) == 1e-3 * (0.1 ** 2)            # resuming past two steps: both are taken at once
    assert lr_at(400000, 1e-3, 0.1, (280000, 360000, 400000), 500, 1e-4) == 1e-3 * (0.1 ** 3)


def test_without_warm_up_and_a_step_inside_it():
    assert lr_at(0, LR, GAMMA, STEPS, 0, INIT) == LR and lr_at(149999, LR, GAMMA, STEPS, 0, INIT) == LR
    assert lr_at(150000, LR, GAMMA, STEPS, 0, INIT) == LR * 0.1
    # the loop sets the warm-up value first and the step's value after it: the step wins
    assert at(300, steps=(200, 400)) == 1e-3 * 0.1 and at(100, steps=(200, 400)) == (1e-3 - 1e-4) * (100 / 500) + 1e-4
    assert lr_at(5, LR, GAMMA, (), UNTIL, INIT) == (1e-3 - 1e-4) * (5 / 500) + 1e-4


def test_autoscale_for_batch_sizes_2_4_8():
    # factor = batch_size * 2 / 8: lr *= factor, max_iter //= factor, lr_steps = [x // factor]
    assert autoscale(1e-3, 250000, (150000, 200000), 2) == (1e-3 * 0.5, 250000 // 0.5, [150000 // 0.5, 200000 // 0.5]) == (5e-4, 500000.0, [300000.0, 400000.0])
    assert autoscale(1e-3, 250000, (150000, 200000), 4) == (1e-3, 250000, (150000, 200000))          # 8 frames per step: untouched
    assert autoscale(1e-3, 250000, (150000, 200000), 8) == (2e-3, 125000.0, [75000.0, 100000.0])
    lr, max_iter, steps = autoscale(1e-3, 250001, (150001, 200001), 8)
    assert (max_iter, steps) == (125000.0, [75000.0, 100000.0])                                        # floor division
    assert autoscale(1e-3, 600000, (280000, 360000, 400000), 3) == (1e-3 * 0.75, 600000 // 0.75, [280000 // 0.75, 360000 // 0.75, 400000 // 0.75])

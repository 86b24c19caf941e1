"""CPU: the epoch schedule of Train.train() (Training/schedule.py; the reference's Training/Train_goodGAN.py:139-146,165-182) on the host,
without a device or a trainer.  Every expectation is written out from the rules: which epoch switches what, and the learning rates as
the running product the loop forms — compared with == on Python floats, since a closed-form power may differ in the last bit."""
import itertools


def records(config, consistency, start_epoch, n):
    """{relative epoch: record} of the first n epochs."""
    from Training.schedule import epoch_schedule
    return dict(zip(range(1, n + 1), itertools.islice(epoch_schedule(config, consistency, start_epoch), n)))


def mnist():
    from Training.Train_goodGAN import MnistConfig
    c = MnistConfig()
    c.PRE_TRAIN = True                               # what _run sets for NUM_LABEL < 1000
    assert (c.LEARNING_RATE, c.CLA_LEARNINIG_RATE, c.FAKE_G_LAMBDA) == (1e-3, 3e-4, 0.1)
    return c


def cifar10():
    from Training.Train_goodGAN import Cifar10Config
    c = Cifar10Config()
    assert (c.LEARNING_RATE, c.CLA_LEARNINIG_RATE, c.FAKE_G_LAMBDA, bool(c.PRE_TRAIN)) == (3e-4, 3e-3, 0.3, False)
    return c


def test_a_record_has_five_named_fields_in_set_hyper_order():
    r = records(cifar10(), True, 0, 1)[1]
    assert r._fields == ('lr', 'cla_lr', 'lambda_1', 'lambda_2', 'pre_train')
    assert tuple(r) == (3e-4, 3e-3, 0., 0., False) and r.pre_train is False


def test_fresh_mnist_run_pre_trains_30_epochs_and_never_has_a_lambda_2():
    r = records(mnist(), False, 0, 302)
    assert all(r[e].pre_train is True for e in range(1, 31)) and r[31].pre_train is False
    assert not any(r[e].pre_train for e in range(31, 303))
    assert r[200].lambda_1 == 0. and r[201].lambda_1 == 0.1
    assert all(r[e].lambda_1 == 0. for e in range(1, 201)) and all(r[e].lambda_1 == 0.1 for e in range(201, 303))
    assert all(r[e].lambda_2 == 0. for e in r)       # consistency = False: at every epoch
    assert all(r[e].lr == 1e-3 and r[e].cla_lr == 3e-4 for e in range(1, 300))
    assert r[300].lr == 1e-3 * 0.995 and r[301].lr == (1e-3 * 0.995) * 0.995
    assert r[300].cla_lr == 3e-4 * 0.99 and r[301].cla_lr == (3e-4 * 0.99) * 0.99


def test_fresh_cifar10_run_switches_lambda_2_on_at_68_and_decays_from_300():
    r = records(cifar10(), True, 0, 302)
    assert not any(r[e].pre_train for e in r)
    assert r[67].lambda_2 == 0. and r[68].lambda_2 == 0.5
    assert all(r[e].lambda_2 == 0. for e in range(1, 68)) and all(r[e].lambda_2 == 0.5 for e in range(68, 303))
    assert r[200].lambda_1 == 0. and r[201].lambda_1 == 0.3
    assert all(r[e].lr == 3e-4 and r[e].cla_lr == 3e-3 for e in range(1, 300))
    assert r[300].lr == 3e-4 * 0.995 and r[301].lr == (3e-4 * 0.995) * 0.995 and r[302].lr == ((3e-4 * 0.995) * 0.995) * 0.995
    assert r[300].cla_lr == 3e-3 * 0.99 and r[301].cla_lr == (3e-3 * 0.99) * 0.99


def test_without_consistency_lambda_2_stays_zero_on_cifar10_too():
    assert all(rec.lambda_2 == 0. for rec in records(cifar10(), False, 0, 302).values())
    assert all(rec.lambda_2 == 0. for rec in records(cifar10(), False, 350, 100).values())


def test_resumed_at_150_lambda_1_follows_the_absolute_epoch_and_lambda_2_the_relative_one():
    r = records(cifar10(), True, 150, 151)
    assert r[50].lambda_1 == 0. and r[51].lambda_1 == 0.3            # absolute epoch 201
    assert all(r[e].lambda_1 == 0.3 for e in range(51, 152))
    assert r[67].lambda_2 == 0. and r[68].lambda_2 == 0.5            # still the 68th epoch of THIS call, absolute epoch 218
    assert all(r[e].lambda_2 == 0. for e in range(1, 68))
    assert r[149].lr == 3e-4 and r[150].lr == 3e-4 * 0.995 and r[151].lr == (3e-4 * 0.995) * 0.995      # absolute 299, 300, 301
    m = mnist()
    assert not any(rec.pre_train for rec in records(m, False, 150, 40).values())       # PRE_TRAIN is set, but epoch 30 is long past
    assert records(m, False, 29, 2)[1].pre_train is True and records(m, False, 29, 2)[2].pre_train is False


def test_resumed_at_350_the_rate_restarts_from_a_power_and_is_decayed_once_more():
    r = records(cifar10(), True, 350, 2)
    assert r[1].lr == (3e-4 * 0.995 ** 50) * 0.995
    assert r[1].cla_lr == (3e-3 * 0.99 ** 50) * 0.99
    assert r[2].lr == ((3e-4 * 0.995 ** 50) * 0.995) * 0.995
    for base, rate, got in ((3e-4, 0.995, r[1].lr), (3e-3, 0.99, r[1].cla_lr)):
        closed = base * rate ** 51
        if closed != (base * rate ** 50) * rate:     # where the two floats differ, the schedule is the product
            assert got != closed
    # nor is it what an uninterrupted run has at absolute epoch 351: 52 multiplications, one per epoch from 300 on
    uninterrupted = records(cifar10(), True, 0, 351)[351].lr
    product = 3e-4
    for _ in range(52):
        product = product * 0.995
    assert uninterrupted == product and r[1].lr != uninterrupted         # 51 factors against 52
    assert r[1].lambda_1 == 0.3 and r[1].lambda_2 == 0. and r[1].pre_train is False


def test_resumed_at_299_and_300_the_first_epoch_is_decayed_once():
    assert records(cifar10(), True, 299, 1)[1].lr == 3e-4 * 0.995
    assert records(cifar10(), True, 299, 1)[1].cla_lr == 3e-3 * 0.99
    assert records(cifar10(), True, 300, 1)[1].lr == (3e-4 * 0.995 ** 0) * 0.995
    assert records(cifar10(), True, 300, 1)[1].cla_lr == (3e-3 * 0.99 ** 0) * 0.99
    assert records(cifar10(), True, 298, 2)[1].lr == 3e-4 and records(cifar10(), True, 298, 2)[2].lr == 3e-4 * 0.995


def test_the_schedule_needs_no_device():
    import torch
    records(mnist(), False, 0, 3)
    assert not torch.cuda.is_initialized()

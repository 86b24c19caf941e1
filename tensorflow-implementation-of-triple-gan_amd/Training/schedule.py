"""The epoch schedule of Train.train() — the reference's Training/Train_goodGAN.py:139-146,165-182 — as a function of the config alone.

No device, no trainer: what an epoch's learning rates, lambdas and pre-training flag are is decided here and can be tested on the host.
The reference's quirks are kept as they are, because a resumed or compared run depends on them:

  * lambda_1 switches on the ABSOLUTE epoch (start_epoch + epoch), lambda_2 on the epoch RELATIVE to this train() call;
  * a restored run's learning rates start at 0.995 ** (start_epoch - 300) and 0.99 ** (start_epoch - 300) of the configured ones, and
    are decayed once more before the first epoch runs — not what an uninterrupted run had at that epoch;
  * the decay is a running product, one multiplication per epoch in this order.  The values reach the device as float32
    (Train.set_hyper), and a closed-form power can differ from the product in the last bit."""
import collections

from Training.options import cla_lr

EpochSchedule = collections.namedtuple('EpochSchedule', 'lr cla_lr lambda_1 lambda_2 pre_train')


def epoch_schedule(config, consistency, start_epoch):
    """yields EpochSchedule(lr, cla_lr, lambda_1, lambda_2, pre_train) for epoch = 1, 2, ... of a train() call that starts behind
    `start_epoch` finished epochs (0: a fresh run).  consistency: the model's CONSISTENCY — only then is lambda_2 ever non-zero."""
    lr, c_lr = config.LEARNING_RATE, cla_lr(config)
    if start_epoch >= 300:                                                             # :143-146
        lr = lr * 0.995 ** (start_epoch - 300)
        c_lr = c_lr * 0.99 ** (start_epoch - 300)
    epoch = 0
    while True:
        epoch += 1
        lambda_1 = config.FAKE_G_LAMBDA if (start_epoch + epoch) > 200 else 0.         # :165
        lambda_2 = (0.5 if epoch > 67 else 0.) if consistency else 0.                  # :171
        if start_epoch + epoch >= 300:                                                 # :175-177
            lr, c_lr = lr * 0.995, c_lr * 0.99
        yield EpochSchedule(lr, c_lr, lambda_1, lambda_2, bool(config.PRE_TRAIN and (start_epoch + epoch <= 30)))   # :182

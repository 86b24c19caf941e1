"""CIFAR-100 counterpart of Input_Pipeline/cifar10Dataset.py: file naming 'cifar100_<subset>_<count:06d>.tfrecords' under
<data_dir>/Tfrecord, train_size 50000, 3 channel(s), pixel scaling x/255*2-1; labels 0..99 (config.NUM_CLASSES = 100).  The pipeline
itself is Input_Pipeline/tfrecordDataset.py."""
from Input_Pipeline.tfrecordDataset import tfrecordDataset


class cifar100Dataset(tfrecordDataset):
    PREFIX = 'cifar100'
    TRAIN_SIZE = 50000
    CHANNELS = 3
    UNIT_RANGE = False
    AUG_SHIFT = 2
    AUG_FLIP = True

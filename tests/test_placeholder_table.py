"""CPU: the one table of the training graph's placeholders (Training/Train_goodGAN.PLACEHOLDERS), which _build_train_graph, feed,
training_statistics and the returned PH list all read."""
import re

KEYS = ('z_g', 'y_g', 'x_l_c', 'y_l_c', 'x_l_d', 'y_l_d', 'x_u_d', 'x_u_c')      # Model.forward_pass's argument order


def test_the_table_names_the_eight_placeholders_in_order():
    from Training.Train_goodGAN import PLACEHOLDERS
    assert tuple(key for key, _, _ in PLACEHOLDERS) == KEYS
    assert all(len(row) == 3 for row in PLACEHOLDERS)
    holds = {key: what for key, _, what in PLACEHOLDERS}
    assert holds['z_g'] == 'latent'
    assert all(holds[k] == ('labels' if k.startswith('y') else 'image') for k in KEYS[1:])
    assert {key: size for key, size, _ in PLACEHOLDERS} == dict(
        z_g='BATCH_SIZE_G', y_g='BATCH_SIZE_G', x_l_c='BATCH_SIZE_L_C', y_l_c='BATCH_SIZE_L_C', x_l_d='BATCH_SIZE_L_D',
        y_l_d='BATCH_SIZE_L_D', x_u_d='BATCH_SIZE_U_D', x_u_c='BATCH_SIZE_U_C')


def test_every_experiment_config_has_each_batch_size_the_table_names():
    from Training import Train_goodGAN as TG
    classes = TG.ExperimentConfig.__subclasses__()
    assert {TG.SvhnConfig, TG.Cifar10Config, TG.Cifar100Config, TG.MnistConfig, TG.Stress64Config} <= set(classes)
    for cls in classes:
        for _, size, _ in TG.PLACEHOLDERS:
            assert isinstance(getattr(cls, size), int) and getattr(cls, size) > 0, (cls.__name__, size)


def test_the_table_holds_the_feed_keys_that_feed_documents():
    from Training.Train_goodGAN import PLACEHOLDERS, Train
    listed = re.search(r'batch keys:\s*([a-z_,\s]+?)\s*\(', Train.feed.__doc__).group(1)
    assert tuple(k.strip() for k in listed.split(',')) == tuple(key for key, _, _ in PLACEHOLDERS)

"""What the models share through Model/model_base.NN_Base, without a device (models construct on the TraceContext of
tests/launch_trace.py): every variant reports its own weight-normalised layers."""
from test_initial_weights import build_model

NIN_AND_HEAD = ('classifier/NiN1/NiN1', 'classifier/NiN2/NiN2', 'classifier/output_dense')


def test_stress64_reports_its_own_weight_normalised_layers(monkeypatch):
    """WN_INIT_LAYERS follows the class's C_CONVS: Good_GAN_stress64 lists conv0_1 ... conv3 (ten convolutions), not CIFAR's seven."""
    from Model.Good_GAN_stress64 import Good_GAN_stress64
    m, _ = build_model('stress64', monkeypatch)
    assert type(m) is Good_GAN_stress64
    names = [row[0] for row in Good_GAN_stress64.C_CONVS]
    assert names == ['conv0_1', 'conv0_2', 'conv0_3', 'conv1_1', 'conv1_2', 'conv1_3', 'conv2_1', 'conv2_2', 'conv2_3', 'conv3']
    layers = m.WN_INIT_LAYERS
    assert layers['classifier'] == tuple('classifier/' + n for n in names) + NIN_AND_HEAD and len(layers['classifier']) == 13
    assert layers['good_generator'] == () and layers['discriminator'] == ()


def test_cifar10_reports_the_ten_layers_it_always_did(monkeypatch):
    m, _ = build_model('cifar10', monkeypatch)
    assert m.WN_INIT_LAYERS == {'good_generator': (), 'discriminator': (),
                                'classifier': ('classifier/conv1_1', 'classifier/conv1_2', 'classifier/conv1_3', 'classifier/conv2_1',
                                               'classifier/conv2_2', 'classifier/conv2_3', 'classifier/conv3') + NIN_AND_HEAD}
    assert len(m.WN_INIT_LAYERS['classifier']) == 10


def test_models_expose_what_the_trainer_reads():
    """Train reads CONSISTENCY and GRAD_BUCKETS as attributes: NN_Base holds the defaults, Good_GAN declares the first."""
    from Model.Good_GAN import Good_GAN
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Model.Good_GAN_stress64 import Good_GAN_stress64
    from Model.model_base import NN_Base
    assert NN_Base.CONSISTENCY is False and NN_Base.GRAD_BUCKETS == {}
    assert Good_GAN.__dict__['CONSISTENCY'] is False and Good_GAN.GRAD_BUCKETS == {}
    assert Good_GAN_cifar10.CONSISTENCY is True and Good_GAN_stress64.CONSISTENCY is True
    assert set(Good_GAN_cifar10.GRAD_BUCKETS) == set(Good_GAN_stress64.GRAD_BUCKETS) == {'classifier', 'good_generator', 'discriminator'}

"""Drop-in for the reference's `lpipsPyTorch` package (imported at metric.py:18): `lpips(x, y, net_type='vgg')` and `LPIPS` over
image_eval.LPIPS.  Only the network the reference uses is built (metric.py:74 passes 'vgg').  The weights come from the two files the
directory RADEGS_LPIPS_WEIGHTS holds (image_eval.load_lpips_weights); nothing is fetched, and the packed network is kept between calls
instead of being rebuilt per call as upstream's functional form does."""
import image_eval


def _only_vgg(net_type, version):
    if version != '0.1':
        raise NotImplementedError("only LPIPS v0.1 is built")
    if net_type != 'vgg':
        raise NotImplementedError(f"only net_type='vgg' is built (what metric.py uses), not {net_type!r}")


class LPIPS(image_eval.LPIPS):
    def __init__(self, net_type='alex', version='0.1'):
        _only_vgg(net_type, version)
        super().__init__(*image_eval.load_lpips_weights())


def lpips(x, y, net_type='alex', version='0.1'):
    _only_vgg(net_type, version)
    return image_eval.default_lpips().forward(x, y)

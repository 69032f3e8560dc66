"""The three argument groups of upstream's scripts (arguments/__init__.py) and get_combined_args.

ParamGroup's rules are upstream's: every attribute set before ParamGroup.__init__ becomes `--name`; a leading underscore also gives the
one-letter shorthand `-n`; a bool is a `store_true` flag; everything else parses with the type of its default; `extract(args)` copies the
group's names from a parsed namespace into a plain object.  The defaults are held to the reference's classes by
tests/golden/trainer_defaults.json (tests/test_trainer_host.py)."""
import os
import sys
from argparse import ArgumentParser, Namespace


class GroupParams:
    pass


class ParamGroup:
    def __init__(self, parser: ArgumentParser, name: str, fill_none=False):
        group = parser.add_argument_group(name)
        for key, value in vars(self).items():
            flags = ["--" + key]
            if key.startswith("_"):
                key = key[1:]
                flags = ["--" + key, "-" + key[0:1]]
            t = type(value)
            default = None if fill_none else value
            if t == bool:
                group.add_argument(*flags, default=default, action="store_true")
            else:
                group.add_argument(*flags, default=default, type=t)

    def extract(self, args):
        group = GroupParams()
        for name, value in vars(args).items():
            if name in vars(self) or ("_" + name) in vars(self):
                setattr(group, name, value)
        return group


class ModelParams(ParamGroup):
    def __init__(self, parser, sentinel=False):
        self.sh_degree = 3
        self._source_path = ""
        self._model_path = ""
        self._images = "images"
        self._dataset = ""
        self._resolution = -1
        self._white_background = False
        self.data_device = "cuda"
        self.eval = False
        self.use_decoupled_appearance = False
        self.use_coord_map = False
        self.disable_filter3D = False
        self.kernel_size = 0.0          # size of the 2D (mip) filter
        super().__init__(parser, "Loading Parameters", sentinel)

    def extract(self, args):
        g = super().extract(args)
        g.source_path = os.path.abspath(g.source_path)
        return g


class PipelineParams(ParamGroup):
    def __init__(self, parser):
        self.convert_SHs_python = False
        self.compute_cov3D_python = False
        self.debug = False
        super().__init__(parser, "Pipeline Parameters")


class OptimizationParams(ParamGroup):
    def __init__(self, parser):
        self.iterations = 30_000
        self.position_lr_init = 0.00016
        self.position_lr_final = 0.0000016
        self.position_lr_delay_mult = 0.01
        self.position_lr_max_steps = 30_000
        self.feature_lr = 0.0025
        self.opacity_lr = 0.05
        self.scaling_lr = 0.005
        self.rotation_lr = 0.001
        self.appearance_embeddings_lr = 0.001
        self.appearance_network_lr = 0.001
        self.percent_dense = 0.01
        self.lambda_dssim = 0.2
        self.lambda_depth_normal = 0.05
        self.densification_interval = 100
        self.opacity_reset_interval = 3000
        self.densify_from_iter = 500
        self.densify_until_iter = 15_000
        self.regularization_from_iter = 15_000
        self.densify_grad_threshold = 0.0002
        super().__init__(parser, "Optimization Parameters")


def read_cfg_args(text):
    """The Namespace a `cfg_args` file holds (it is `str(Namespace(...))`): evaluated with `Namespace` as the only name in scope and no
    builtins, so the file can construct a Namespace of literals and nothing else."""
    ns = eval(text, {"__builtins__": {}, "Namespace": Namespace}, {})      # noqa: S307
    if not isinstance(ns, Namespace):
        raise RuntimeError("cfg_args does not hold a Namespace")
    return ns


def get_combined_args(parser: ArgumentParser, argv=None):
    """The command line merged over <model_path>/cfg_args: a value given on the command line (anything that is not None) wins.  Meant for
    parsers whose ModelParams were made with sentinel=True, as upstream's render.py does."""
    args_cmdline = parser.parse_args(sys.argv[1:] if argv is None else argv)
    cfgfile_string = "Namespace()"
    try:
        cfgfilepath = os.path.join(args_cmdline.model_path, "cfg_args")
        print("Looking for config file in", cfgfilepath)
        with open(cfgfilepath) as cfg_file:
            print("Config file found: {}".format(cfgfilepath))
            cfgfile_string = cfg_file.read()
    except TypeError:
        print("Config file not found at")
    merged = vars(read_cfg_args(cfgfile_string)).copy()
    for k, v in vars(args_cmdline).items():
        if v is not None:
            merged[k] = v
    return Namespace(**merged)


def install():
    """Registers this module as `arguments`, so that upstream's `from arguments import ModelParams, ...` resolves to it.  Opt-in: nothing
    calls it."""
    sys.modules["arguments"] = sys.modules[__name__]
    return sys.modules[__name__]

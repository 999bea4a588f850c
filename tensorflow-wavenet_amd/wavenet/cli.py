"""What train.py, generate.py and evaluate.py share on the command line."""


def str_to_bool(s):
    if s.lower() not in ('true', 'false'):
        raise ValueError('Argument needs to be a boolean, got {}'.format(s))
    return s.lower() == 'true'


def model_from_params(wavenet_params, batch_size, **conditioning):
    """The WaveNetModel of a wavenet_params.json dict.  `conditioning`: the
    keywords the command line decides instead (global_condition_*,
    local_condition_*, histograms)."""
    # (looked up at the call: a test may have put a stub in its place)
    from . import WaveNetModel
    return WaveNetModel(
        batch_size=batch_size,
        dilations=wavenet_params['dilations'],
        filter_width=wavenet_params['filter_width'],
        residual_channels=wavenet_params['residual_channels'],
        dilation_channels=wavenet_params['dilation_channels'],
        skip_channels=wavenet_params['skip_channels'],
        quantization_channels=wavenet_params['quantization_channels'],
        use_biases=wavenet_params['use_biases'],
        scalar_input=wavenet_params['scalar_input'],
        initial_filter_width=wavenet_params['initial_filter_width'],
        residual_postproc=wavenet_params.get('residual_postproc', False),
        **conditioning)


PIECE_HISTORY_HELP = (
    'Put up to this many samples of a piece\'s true left context in front of '
    'it: they are fed to the network but not predicted (WaveNetModel.loss, '
    'history=), so every predicted sample sees the history it sees at '
    'generation time.  N samples, or rf = the model\'s receptive field.  '
    'Default: off (a piece\'s first samples see zeros).')


def piece_history_arg(s):
    """argparse type of --piece_history: 'rf' or a non-negative int."""
    if s == 'rf':
        return s
    try:
        n = int(s)
    except ValueError:
        n = -1
    if n < 0:
        raise ValueError('--piece_history takes a non-negative int or rf, '
                         'got {}'.format(s))
    return n


def piece_history(value, wavenet_params):
    """The samples of --piece_history (None: 0) for a wavenet_params.json
    dict: 'rf' is WaveNetModel.receptive_field of that model."""
    if value is None:
        return 0
    if value != 'rf':
        return int(value)
    from .model import receptive_field
    return receptive_field(wavenet_params['dilations'],
                           wavenet_params['filter_width'],
                           wavenet_params['scalar_input'],
                           wavenet_params['initial_filter_width'])

"""Where a run's configuration comes from (reference: utils/config.py, same function names).

A training run leaves ``config/config.json`` and ``config/args.json`` beside its ``checkpoints`` directory; the tools that take
a checkpoint read both (the arguments win over the file's entries), or one JSON / YAML file given in their place.
``load_yaml_config`` and ``merge_config_and_args``, which the reference keeps in the same module, are train.py's here.
"""
import json
from pathlib import Path
from typing import Optional, Union


def load_config_from_alternative_file(config_path: Union[str, Path], checkpoint_path: Optional[str],
                                      insert_stylegan_checkpoint: bool = False) -> dict:
    config_path = Path(config_path)
    if config_path.suffix == '.json':
        with config_path.open() as f:
            config = json.load(f)
    elif config_path.suffix == '.yaml':
        import yaml
        with config_path.open() as f:
            config = yaml.safe_load(f)
    else:
        raise NotImplementedError(f"{config_path}: a .json or .yaml config is needed")
    if insert_stylegan_checkpoint:
        if checkpoint_path is not None:
            config['stylegan_checkpoint'] = checkpoint_path
        assert config.get('stylegan_checkpoint') is not None, "the config names no stylegan_checkpoint and none was given"
    return config


def load_config_from_checkpoint(checkpoint_path: Union[str, Path]) -> dict:
    config_dir = Path(checkpoint_path).parent.parent / 'config'
    try:
        with (config_dir / 'config.json').open() as f:
            config = json.load(f)
        with (config_dir / 'args.json').open() as f:
            config.update(json.load(f))
    except FileNotFoundError as err:
        raise FileNotFoundError(f"{config_dir} must hold the run's config.json and args.json (two levels above the checkpoint); "
                                "otherwise pass the config file itself") from err
    return config


def load_config(checkpoint_path: Optional[str] = None, config_path: Union[str, Path, None] = None,
                insert_stylegan_checkpoint: bool = False) -> dict:
    if checkpoint_path is None and config_path is None:
        raise RuntimeError("You have to supply either checkpoint path or path to a config file!")
    if config_path is not None:
        return load_config_from_alternative_file(config_path, checkpoint_path, insert_stylegan_checkpoint)
    return load_config_from_checkpoint(checkpoint_path)


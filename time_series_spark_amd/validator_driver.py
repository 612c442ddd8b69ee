"""`python -m time_series_spark_amd.validator_driver config.yaml` -- cross-validate every (series_id, dim_id) of the
modeler's input directory on the GPU and write the per-series metrics parquet (jobs/prophet_validator.py); the
config is the modeler's (io.input, model.*) plus io.metrics, optionally io.folds, and the `cv` settings."""
import sys

import yaml

from .jobs.prophet_validator import ProphetValidator


def main(argv=None):
    argv = sys.argv if argv is None else argv
    if len(argv) != 2:
        print("arg1 must be the config YAML")
        return 1
    with open(argv[1]) as file:
        config = yaml.safe_load(file)
    print(f"config: {config}")
    ProphetValidator.validate(None, config, return_frame=False)
    return 0


if __name__ == '__main__':
    sys.exit(main())

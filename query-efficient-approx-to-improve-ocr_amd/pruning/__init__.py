"""Dataset pruning (the reference's pruning/): pick the training documents worth their OCR queries (methods.py) and write the
artifact that `patch_cli.py --pruning_artifact NAME` trains on (prune_dataset.py)."""

"""Generate tests/golden/traj_augmentation_schema.json: model_dump() of the reference's TrajAugmentationSchema defaults.

Run where the reference checkout is (its path: the first argument, or the environment variable
DEEP_CARTOGRAPH_REFERENCE); it never travels with this repository:

    python tests/golden/make_golden_traj_augmentation.py <reference checkout>

What is stored is *data* (field names and default values), never reference source.
"""
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DEEP_CARTOGRAPH_REFERENCE")
    if not ref:
        sys.exit("give the path of the reference checkout")
    sys.path.insert(0, ref)
    from deep_cartograph.yaml_schemas.traj_augmentation import TrajAugmentationSchema

    dump = TrajAugmentationSchema().model_dump()
    with open(os.path.join(OUT, "traj_augmentation_schema.json"), "w") as f:
        json.dump(dump, f, indent=1, sort_keys=True)
        f.write("\n")
    print("traj_augmentation_schema.json:", dump)


if __name__ == "__main__":
    main()

"""Drop-in for the reference's data_utils.py (`import data_utils`, localize.py:11)."""
from piccolo_amd.data_utils import (load_cloud, obtain_align_matrix, obtain_gt_omniscenes, obtain_gt_stanford,  # noqa: F401
                                    read_omniscenes, read_stanford)

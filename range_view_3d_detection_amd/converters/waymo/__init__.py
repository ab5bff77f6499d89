from .utils import (batch_from_range_images, compute_inclination, inclinations_by_row, labels_to_annotations, range_image_to_sweep, sweep_table,  # noqa: F401
                    write_sweep)

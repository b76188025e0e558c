"""Built-in scalar functions (functions/mod.rs, functions/datetime/extract.rs). As in the reference, a function is named and
typed on the host; here its evaluation is generated into the HIP kernels of the plan (csrc/device/qhip_datetime.inc for
EXTRACT) instead of an ``eval`` over Arrow arrays."""
from __future__ import annotations

from typing import List

import pyarrow as pa

# qhip_function (include/qhip.h)
FN_EXTRACT = 0


class UserDefinedFunction:
    """trait UserDefinedFunction (functions/mod.rs:9-20)."""
    fn_id = -1

    def name(self) -> str:
        raise NotImplementedError

    def return_type(self) -> pa.DataType:
        raise NotImplementedError

    def is_nullable(self) -> bool:
        return True

    def __repr__(self):
        return self.name()


class DatetimeExtract(UserDefinedFunction):
    """functions/datetime/extract.rs: EXTRACT(part FROM date / timestamp) -> Int64, args = [Utf8 part, value]."""
    fn_id = FN_EXTRACT

    def name(self) -> str:
        return "EXTRACT"

    def return_type(self) -> pa.DataType:
        return pa.int64()


def all_builtin_functions() -> List[UserDefinedFunction]:
    """functions/mod.rs:22-24"""
    return [DatetimeExtract()]

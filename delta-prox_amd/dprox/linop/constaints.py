"""The pieces a linear program is written with (reference dprox/linop/constaints.py, whose file name is kept):
``c @ x`` is a ``matmul``, ``A @ x <= b`` a ``less`` and ``A @ x == b`` an ``equality``; ``Problem`` reads them."""


class matmul:
    def __init__(self, var, A):
        self.A = A
        self.var = var

    def __eq__(self, other):
        return equality(self, other)

    def __le__(self, other):
        return less(self, other)

    __hash__ = None


class equality:
    def __init__(self, left: matmul, right):
        self.left = left
        self.right = right


class less:
    def __init__(self, left: matmul, right):
        self.left = left
        self.right = right

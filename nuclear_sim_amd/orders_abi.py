"""include/npb.h npb_control_order_t, npb_control_orders_desc_t: order rules on the controls' VALUE axes (npb_set_control_orders) as the
binding passes them.  tests/test_control_orders_abi.py holds the layout to the compiler's."""
import ctypes

CONTROL_ORDERS_MAX = 8                                                 # NPB_CONTROL_ORDERS_MAX (controls.ORDERS_MAX)
CONTROL_ORDER_NEVER = 0x7fffffff                                       # NPB_CONTROL_ORDER_NEVER (controls.NEVER)
ORDER_FAMILIES = {"pump": 0, "component": 1, "turbine": 2}             # NPB_ORDER_* (controls.FAMILIES)


class NpbControlOrder(ctypes.Structure):
    """npb_control_order_t: one rule, the axis it reads and the service it orders"""
    _fields_ = [("axis", ctypes.c_int), ("family", ctypes.c_int), ("action", ctypes.c_int), ("unit", ctypes.c_int), ("option", ctypes.c_int),
                ("min_interval", ctypes.c_int), ("amount", ctypes.c_double), ("threshold", ctypes.c_double)]


class NpbControlOrdersDesc(ctypes.Structure):
    """npb_control_orders_desc_t: the rules (a host array) and the caller's device ``fired`` [n_orders][n_plants]"""
    _fields_ = [("n_orders", ctypes.c_int), ("orders", ctypes.POINTER(NpbControlOrder)), ("fired", ctypes.c_void_p)]

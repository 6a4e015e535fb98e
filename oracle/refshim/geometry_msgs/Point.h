// Stand-in message struct (TEST INFRASTRUCTURE ONLY; see ../ros/ros.h).
#ifndef F110_REFSHIM_POINT_H
#define F110_REFSHIM_POINT_H
namespace geometry_msgs {
struct Point { double x = 0, y = 0, z = 0; };
}
#endif

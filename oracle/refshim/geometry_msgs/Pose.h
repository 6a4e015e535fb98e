// Stand-in message struct (TEST INFRASTRUCTURE ONLY; see ../ros/ros.h).
#ifndef F110_REFSHIM_POSE_H
#define F110_REFSHIM_POSE_H
#include "Point.h"
namespace geometry_msgs {
struct Quaternion { double x = 0, y = 0, z = 0, w = 0; };
struct Pose { Point position; Quaternion orientation; };
}
#endif

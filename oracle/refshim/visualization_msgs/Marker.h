// Stand-in message struct (TEST INFRASTRUCTURE ONLY; see ../ros/ros.h).
#ifndef F110_REFSHIM_MARKER_H
#define F110_REFSHIM_MARKER_H
#include <string>
#include <vector>
#include "../geometry_msgs/Pose.h"
#include "../ros/ros.h"
#include "../std_msgs/ColorRGBA.h"
namespace visualization_msgs {
struct Marker {
  enum { ARROW = 0, CUBE = 1, SPHERE = 2, CYLINDER = 3, LINE_STRIP = 4, LINE_LIST = 5, CUBE_LIST = 6, SPHERE_LIST = 7 };
  enum { ADD = 0, MODIFY = 0, DELETE = 2 };
  struct Header { std::string frame_id; ros::Time stamp; } header;
  std::string ns;
  int id = 0, type = 0, action = 0;
  geometry_msgs::Pose pose;
  struct Scale { double x = 0, y = 0, z = 0; } scale;
  std_msgs::ColorRGBA color;
  std::vector<geometry_msgs::Point> points;
  std::vector<std_msgs::ColorRGBA> colors;
};
}
#endif
